/* balatro_mi355x.h -- C ABI of the MI355X-native vectorised Balatro environment (libbalatro_mi355x.so).
 *
 * This is the drop-in boundary for ONE hot path of cassiusfive/balatro-gym: the step()/reset() loop of
 * `balatro_gym/balatro_env_2.py::BalatroEnv` (deck shuffle/draw -> hand classification -> chip/mult accumulation ->
 * joker chain -> planet-level / boss-blind multipliers -> blind outcome -> observation + action mask).  The reference
 * is pure Python with no FFI; the entry points below are what a ctypes binding on the reference side would call
 * (see INTEGRATION.md).  Each entry point cites the reference interface it replaces (paths relative to the
 * reference's balatro_gym/ directory).
 *
 * Conventions: plain C, no torch types; every function returns 0 on success and a negative BG_E_* code on failure
 * (bg_last_error() gives the text); all `*_dev` pointers are DEVICE pointers into buffers the CALLER owns (e.g.
 * torch tensors' data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream); the library owns
 * the per-env game/RNG state (structure-of-arrays in HBM) and never synchronises the host inside bg_step /
 * bg_rollout.  One handle drives one GPU; a handle is not thread-safe, different handles are independent.
 * There is NO CPU fallback: without a HIP device bg_create fails.
 */
#ifndef BALATRO_MI355X_H
#define BALATRO_MI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BG_NUM_ACTIONS 60 /* constants.py:117 ACTION_SPACE_SIZE */
#define BG_OBS_BYTES 330  /* bytes of one observation in the reference's dtypes */

/* bg_create flags */
#define BG_FLAG_SCORER_JOKERS 1u /* hand the scorer joker NAMES (unified_scoring.py:313-351) so the joker chain is live */
#define BG_FLAG_AUTORESET 2u     /* SAME_STEP auto-reset: a terminated env is reset() inside the same bg_step call */
#define BG_FLAG_CARD_STATES 4u  /* keep cards.py CardState (enhancement / edition / seal) per deck index: bg_inject_cards */

/* error codes */
#define BG_E_ARG (-1)
#define BG_E_HIP (-2)
#define BG_E_NODEVICE (-3)
#define BG_E_INTERNAL (-4) /* device-side invariant violated (RNG look-ahead ring underflow); sticky */

/* info.error values (device side) -- reference error strings in brackets */
#define BG_ERR_NONE 0
#define BG_ERR_INVALID_ACTION 1 /* balatro_env_2.py:627 'Invalid action' */
#define BG_ERR_PSYCHIC 2        /* boss_blinds.py:388 'Must play exactly 5 cards' */
#define BG_ERR_EYE 3            /* boss_blinds.py:393 'Cannot play <type> again' */
#define BG_ERR_MOUTH 4          /* boss_blinds.py:399 'Can only play <type>' */
#define BG_ERR_VERDANT 5        /* boss_blinds.py:405 'Must play at least <n> cards' */
#define BG_ERR_REROLL_FUNDS 6   /* shop.py:173 'Insufficient chips for reroll' */
#define BG_ERR_JOKER_SLOTS 7    /* shop.py:196 'Joker slots full' */
#define BG_ERR_CONSUMABLE 8     /* balatro_env_2.py:1166-1168 the consumable had no effect (result['success'] False), reward -1.0 */
#define BG_ERR_MAX_ANTE 9       /* balatro_env_2.py:620 terminated 'max_ante_reached' */
#define BG_ERR_MAX_SCORE 10     /* balatro_env_2.py:623 terminated 'max_score_reached' */
#define BG_ERR_CONSUMABLE_RAISES 11 /* the reference RAISES here (consumables.py:246,381,418,444 list.remove of a target class;
                                     * :496,506 assignment to a frozen dataclass): reward -1.0, state as the exception leaves it */
#define BG_ERR_CONSUMABLE_DECK 12   /* Immolate on a deck of fewer than 13 real cards (consumables.py:519-531: fewer than 8 would be left, and the
                                     * hand's deck indexes 0..7 go stale -- the reference's unguarded deck[i] reads, balatro_env_2.py:577,670,937,
                                     * raise from there on) / a Cryptid that would make the deck 128 cards (:581-591: deck_size is
                                     * np.int8(len(deck)), :1491 -- OverflowError under numpy >= 2, a wrapped value under numpy 1);
                                     * reward -1.0, state untouched */

/* info.flags bits */
#define BG_INFO_BEAT_BLIND 1     /* info['beat_blind'] */
#define BG_INFO_FAILED 2         /* info['failed'] */
#define BG_INFO_SKIPPED_BLIND 4  /* info['skipped_blind'] */
#define BG_INFO_OPENED_PACK 8    /* info['opened_pack'] */
#define BG_INFO_BOUGHT_CARD 16   /* info['bought_card'] */
#define BG_INFO_BOUGHT_VOUCHER 32
#define BG_INFO_BOUGHT_JOKER 64
#define BG_INFO_SOLD_JOKER 128   /* info['sold_joker'] (aux = joker id) */
#define BG_INFO_CURRICULUM 256   /* info['curriculum_limit_reached'] (train_balatro_agent.py:146-152) */
#define BG_INFO_AUTORESET 512    /* the env was reset inside this step (BG_FLAG_AUTORESET) */

/* policies of bg_rollout (counter-hash random policy) */
#define BG_POLICY_UNIFORM 0    /* k-th valid action, k = hash(seed, env, t) mod n_valid */
#define BG_POLICY_SMALL_ONLY 1 /* BLIND_SELECT->45, SHOP->31, else uniform (balatro_env_2.py:1841-1849) */
#define BG_POLICY_CYCLE3 2     /* BLIND_SELECT->45+env%3, SHOP->31, else uniform */
#define BG_POLICY_HASH_OBS 0x100 /* OR into `policy`: also fold every observation row into stats.obs_hash (tests) */

typedef struct bg_handle bg_handle;

/* Observation: one device pointer per key of BalatroEnv._get_observation() (balatro_env_2.py:1488-1531), each a
 * contiguous [n_envs, ...] array in the REFERENCE's dtype.  A NULL pointer skips that key. */
typedef struct bg_obs_ptrs {
  int8_t* hand;                 /* [N,8]  int8, -1 padded */
  int8_t* hand_size;            /* [N] */
  int8_t* deck_size;            /* [N] */
  int64_t* selected_cards;      /* [N,8]  int64 0/1 (the reference emits int64 here) */
  int64_t* chips_scored;        /* [N] */
  int32_t* round_chips_scored;  /* [N] */
  float* progress_ratio;        /* [N] */
  int32_t* mult;                /* [N] always 1 */
  int32_t* chips_needed;        /* [N] */
  int32_t* money;               /* [N] */
  int16_t* ante;                /* [N] */
  int8_t* round;                /* [N] */
  int8_t* hands_left;           /* [N] */
  int8_t* discards_left;        /* [N] */
  int8_t* joker_count;          /* [N] */
  int16_t* joker_ids;           /* [N,10] */
  int8_t* joker_slots;          /* [N] */
  int8_t* consumable_count;     /* [N] */
  int16_t* consumables;         /* [N,5] */
  int8_t* consumable_slots;     /* [N] */
  int16_t* shop_items;          /* [N,10] */
  int16_t* shop_costs;          /* [N,10] */
  int16_t* shop_rerolls;        /* [N] */
  int8_t* hand_levels;          /* [N,12] */
  int8_t* phase;                /* [N] */
  int8_t* action_mask;          /* [N,60] */
  int32_t* hands_played;        /* [N] */
  int32_t* best_hand_this_ante; /* [N] */
  int8_t* boss_blind_active;    /* [N] */
  int8_t* boss_blind_type;      /* [N] */
  int64_t* face_down_cards;     /* [N,8] int64 0/1 */
} bg_obs_ptrs;

/* Per-step info (the numeric content of the reference's info dict, balatro_env_2.py:895-925).  NULL skips. */
typedef struct bg_info_ptrs {
  int64_t* final_score;  /* [N] info['final_score'] on an accepted play, else 0 */
  int32_t* error;        /* [N] BG_ERR_* */
  int32_t* flags;        /* [N] BG_INFO_* */
  int32_t* aux;          /* [N] boss type on action 47 / joker id bought or sold / first pack card; on a boss rejection what the reference's
                          * message names (boss_blinds.py:393,399,405): BG_ERR_EYE the hand type played again, BG_ERR_MOUTH the one allowed
                          * hand type, BG_ERR_VERDANT the number of cards required */
  int8_t* hand_type;     /* [N] info['hand_type'] on an accepted play, else -1 */
  int8_t* cards_played;  /* [N] info['cards_played'] */
  double* reward_terms;  /* [N,8] info['reward_breakdown'] without 'total' */
  double* score_breakdown; /* [N,8] info['score_breakdown'] of an accepted play (balatro_env_2.py:909, unified_scoring.py:129-137,293-297):
                          * final_chips, final_mult, final_x_mult, card_chips, base_chips, base_mult, money_gained, 0 (integers are exact:
                          * below 2**53); joker_chips = final_chips - base_chips - card_chips, joker_mult = final_mult - base_mult,
                          * joker_x_mult = final_x_mult.  Zeros on every other step. */
} bg_info_ptrs;

/* Aggregate counters of a rollout (device, one struct per call; all ranks of a sharded job sum them on the host). */
typedef struct bg_rollout_stats {
  uint64_t steps;        /* env-steps executed */
  uint64_t episodes;     /* terminated episodes */
  uint64_t plays;        /* accepted PLAY_HAND steps */
  int64_t score_sum;     /* sum of final_score over accepted plays */
  uint64_t reward_bits;  /* XOR of the IEEE bit patterns of all rewards (order-independent checksum) */
  uint64_t obs_hash;     /* XOR over (env,t) of a 64-bit hash of each observation row (only with BG_POLICY_HASH_OBS) */
} bg_rollout_stats;

/* Identity of the device code: sha256 prefix over the sources, compiler flags and compiler version the library was built from
 * ("unsigned" for ad-hoc builds).  Reproducible across rebuilds of unchanged sources -- the bytes of the code object are not --, so
 * profiles/rNN_hbm_traffic.json measurements are keyed on it (bench.py roofline.traffic).  No reference counterpart. */
const char* bg_build_signature(void);

/* Replaces: constructing n_envs `BalatroEnv` objects (balatro_env_2.py:359-384) + SB3 SubprocVecEnv (hpc_train.py:60-65).
 * max_ante > 0 applies the CurriculumBalatroEnv cap (train_balatro_agent.py:146-152) to every env; bg_set_max_ante changes it
 * later.  Every entry point runs on the handle's device and leaves the caller's current device unchanged. */
int bg_create(int n_envs, int device_id, uint32_t flags, int max_ante, bg_handle** out);
/* bg_create with a memory hint: fused_steps_hint = the most steps the caller will ever ask ONE launch to fuse (bg_step users: 1;
 * an SB3-style collector: its n_steps; 0 = the default, 372-step launches).  The RNG look-ahead rings -- 0.2 MB per env at
 * full depth, 12.8 GB at 65 536 envs -- are sized for that: hint 16 -> 26 KB per env, hint 64 -> 46 KB (bg_state_bytes tells).
 * bg_max_fused_steps reports what the rings allow; longer bg_rollout / bg_step_many calls are split into several launches. */
int bg_create_ex(int n_envs, int device_id, uint32_t flags, int max_ante, int fused_steps_hint, bg_handle** out);
/* Replaces: `CurriculumBalatroEnv.current_max_ante` (train_balatro_agent.py:129-166: one wrapper, hence one cap, per env; the
 * cap rises by ante_increment when 80 % of the last 100 episodes reached it).  The cap is part of an env's state: it survives
 * reset() and travels in state blobs.  per_env_host == NULL sets `max_ante` for the masked envs (mask_host NULL = all),
 * otherwise per_env_host[i]; 0 = no cap; caps are in [0, 255].  The host decides WHEN to raise a cap (the statistics it needs
 * are the terminated flags and the ante of the finished episodes); see balatro_gym_amd/sb3_adapter.py CurriculumTracker.
 * A new cap is checked against the env's reset template only, so it may be LOWERED below the ante of a running env.  As in the reference
 * (train_balatro_agent.py:147-152: `state.ante > current_max_ante` is tested on every step), such an env ends its episode on its NEXT
 * step, whatever the action -- a card toggle, a shop leave or a rejected action included: terminated = 1, BG_INFO_CURRICULUM (256) in the
 * info flags, the reward the action earns, and the reset under auto-reset.  With auto-reset off the env stays above its cap and every
 * further step reports the same until the caller resets it.  This holds on every step path: bg_step, bg_step_rows, bg_step_many,
 * bg_step_many_rows (with limits and progression rewards too), bg_rollout and bg_rollout_rows. */
int bg_set_max_ante(bg_handle* h, int max_ante, const int32_t* per_env_host /*[N] or NULL*/, const uint8_t* mask_host, void* stream);
int bg_destroy(bg_handle* h);
const char* bg_last_error(const bg_handle* h); /* also valid with h == NULL after a failed bg_create */
int bg_num_envs(const bg_handle* h);
/* Largest T that bg_rollout runs as ONE kernel launch (longer rollouts are split into launches of this many steps, with
 * an RNG look-ahead refill between them).  Size [T, N] observation buffers to a multiple of it. */
int bg_max_fused_steps(const bg_handle* h);
uint64_t bg_state_bytes(const bg_handle* h); /* HBM held by the library for this handle */

/* Replaces: `DeterministicRNG(seed)` (balatro_env_2.py:84-106) for the masked envs; seeds_host[i] is env i's master seed,
 * mask_host (nullable = all) selects envs.  reseed_global != 0 also seeds the per-env stand-in for the process-global
 * `random` module with G(seed) = (seed + 16000) mod 2**32 (harness convention).  Does NOT reset the game. */
int bg_seed(bg_handle* h, const int64_t* seeds_host, const uint8_t* mask_host, int reseed_global, void* stream);

/* Replaces: `BalatroEnv.reset()` without a seed (balatro_env_2.py:505-558) for the envs with mask_dev[i] != 0
 * (NULL = all) and writes the observation of EVERY env. */
int bg_reset(bg_handle* h, const uint8_t* mask_dev, const bg_obs_ptrs* obs, void* stream);

/* Replaces: `BalatroEnv.step(action)` (balatro_env_2.py:616-637) for all envs in lockstep.  Invalid actions give
 * reward -1.0 / info.error exactly like the reference; nothing raises. */
int bg_step(bg_handle* h, const int32_t* actions_dev, const bg_obs_ptrs* obs, double* reward_dev,
            uint8_t* terminated_dev, uint8_t* truncated_dev, const bg_info_ptrs* info, void* stream);

/* K consecutive `step()` calls per env in ONE launch: actions_dev is [K, N] (row k = the actions of call k), and with
 * obs_stride_steps != 0 every output is a [K, N, ...] buffer (row k = what call k returned); with 0 the [N, ...] buffers are
 * overwritten and hold the last call's values.  Identical to K bg_step calls (same auto-reset rule, same info), without K
 * launches.  Replaces the inner loop of an SB3-style rollout collection when the actions of several steps are known up front
 * (scripted policies, replay, open-loop evaluation); hpc_train.py:60-65 / balatro_env_2.py:616-637. */
int bg_step_many(bg_handle* h, int K, const int32_t* actions_dev, const bg_obs_ptrs* obs, int obs_stride_steps, double* reward_dev,
                 uint8_t* terminated_dev, uint8_t* truncated_dev, const bg_info_ptrs* info, void* stream);

/* Replaces: `_get_observation()` / `_get_action_mask()` (balatro_env_2.py:1426-1541) without stepping. */
int bg_observe(bg_handle* h, const bg_obs_ptrs* obs, void* stream);

/* bg_step / bg_observe with the observation as ONE packed record per env (the BG_ROW_* layout of bg_rollout_rows below: every key a
 * strided view of a [N, row_stride_bytes] byte tensor, plus the step's reward / action / terminated) instead of 31 arrays: what a
 * policy network reads after `obs_as_tensor` + concatenation anyway.  A cheap step then patches the record image and the copier waves
 * write it (a step that emits 31 arrays spends most of its instructions on address arithmetic): the one-step launch is ~10 % shorter (19.5 against 21.6 us of kernel time at 65 536 envs: bench.py step_path).
 * Same step semantics, same reward / terminated / truncated / info arrays as bg_step (balatro_env_2.py:616-637, :1473-1541);
 * bg_observe_rows (bytes 352.. of a record untouched; the record's reward / action / terminated written as 0) after bg_reset(h, mask, NULL, stream)
 * gives the records of a reset.
 * rows_dev: 16-byte aligned, row_stride_bytes a multiple of 16, >= BG_ROW_BYTES; BG_RECORD_STRIDE_LINES on a 128-byte aligned buffer is the fast layout. */
int bg_step_rows(bg_handle* h, const int32_t* actions_dev, uint8_t* rows_dev, uint64_t row_stride_bytes, double* reward_dev,
                 uint8_t* terminated_dev, uint8_t* truncated_dev, const bg_info_ptrs* info, void* stream);
int bg_observe_rows(bg_handle* h, uint8_t* rows_dev, uint64_t row_stride_bytes, void* stream);

/* Fused random-policy rollout: T steps of every env with the counter-hash policy computed on device and SAME_STEP
 * auto-reset, observations of step t written to row t of [T, N, ...] buffers when obs_stride_steps != 0 (or
 * overwritten in place when 0).  env_index0 = global index of this handle's env 0 (sharding); t0 = first step number.
 * Replaces the driver loop of balatro_env_2.py:1835-1859 / SB3 rollout collection. */
int bg_rollout(bg_handle* h, int T, int policy, uint64_t policy_seed, uint64_t env_index0, uint64_t t0,
               const bg_obs_ptrs* obs, int obs_stride_steps, double* reward_dev, uint8_t* terminated_dev,
               int32_t* actions_out_dev, bg_rollout_stats* stats_dev, void* stream);

/* bg_rollout with ONE packed record per (step, env) instead of one array per key: record (t, i) starts at
 * rows_dev + ((t * rows_stride_steps ? t : 0) * N + i) * row_stride_bytes, i.e. a [T, N, row_stride_bytes] byte tensor
 * when rows_stride_steps != 0 (a [N, row_stride_bytes] tensor overwritten every step when 0).  Every field keeps the
 * reference's dtype at a naturally aligned offset (BG_ROW_*), so each key is a strided view of the same buffer; the
 * step's reward, action and terminated flag ride in the record.  A record is written by one lane with whole 16-byte
 * stores, which keeps HBM write traffic at the record size however far the envs of a workgroup drift apart in time.
 * rows_dev must be 16-byte aligned, row_stride_bytes a multiple of 16 and >= BG_ROW_BYTES.
 * FAST LAYOUT: row_stride_bytes == BG_RECORD_STRIDE_LINES (384) with rows_dev 128-byte aligned.  The library then writes every record as
 * three WHOLE 128-byte lines (bytes 352..383 as zeros): the MI355X's HBM takes records scattered over a buffer at 4.5 TB/s when their
 * lines are written completely and at 2.6 TB/s when each record ends in partial lines, which is what bounds a fused rollout
 * (tools/micro/recwrite.hip).  With any other stride bytes 352.. of a record are left untouched. */
#define BG_ROW_BYTES 352
#define BG_RECORD_STRIDE_LINES 384
#define BG_ROW_SELECTED_CARDS 0       /* int64[8] */
#define BG_ROW_FACE_DOWN_CARDS 64     /* int64[8] */
#define BG_ROW_CHIPS_SCORED 128       /* int64 */
#define BG_ROW_REWARD 136             /* float64: reward of this step */
#define BG_ROW_ROUND_CHIPS_SCORED 144 /* int32 */
#define BG_ROW_PROGRESS_RATIO 148     /* float32 */
#define BG_ROW_MULT 152               /* int32 */
#define BG_ROW_CHIPS_NEEDED 156       /* int32 */
#define BG_ROW_MONEY 160              /* int32 */
#define BG_ROW_HANDS_PLAYED 164       /* int32 */
#define BG_ROW_BEST_HAND_THIS_ANTE 168 /* int32 */
#define BG_ROW_ACTION 172             /* int32: action taken at this step */
#define BG_ROW_ACTION_MASK 176        /* int8[60] */
#define BG_ROW_JOKER_IDS 236          /* int16[10] */
#define BG_ROW_SHOP_ITEMS 256         /* int16[10] */
#define BG_ROW_SHOP_COSTS 276         /* int16[10] */
#define BG_ROW_CONSUMABLES 296        /* int16[5] */
#define BG_ROW_ANTE 306               /* int16 */
#define BG_ROW_SHOP_REROLLS 308       /* int16 */
#define BG_ROW_HAND 310               /* int8[8] */
#define BG_ROW_HAND_LEVELS 318        /* int8[12] */
#define BG_ROW_HAND_SIZE 330          /* int8; the following scalars are int8 each */
#define BG_ROW_DECK_SIZE 331
#define BG_ROW_ROUND 332
#define BG_ROW_HANDS_LEFT 333
#define BG_ROW_DISCARDS_LEFT 334
#define BG_ROW_JOKER_COUNT 335
#define BG_ROW_JOKER_SLOTS 336
#define BG_ROW_CONSUMABLE_COUNT 337
#define BG_ROW_CONSUMABLE_SLOTS 338
#define BG_ROW_PHASE 339
#define BG_ROW_BOSS_BLIND_ACTIVE 340
#define BG_ROW_BOSS_BLIND_TYPE 341
#define BG_ROW_TERMINATED 342         /* uint8: the step ended the episode (SAME_STEP auto-reset: the record already shows the new episode) */
int bg_rollout_rows(bg_handle* h, int T, int policy, uint64_t policy_seed, uint64_t env_index0, uint64_t t0,
                    uint8_t* rows_dev, uint64_t row_stride_bytes, int rows_stride_steps, bg_rollout_stats* stats_dev,
                    void* stream);

/* K consecutive step() calls per env with the CALLER's actions, on the packed-record engine of bg_rollout_rows (bg_engine3.h: owner waves +
 * service waves per workgroup): what bg_step_many does, at the rollout's rate, for callers whose actions come from a network.
 * Replaces: K calls of `BalatroEnv.step(action)` per env (balatro_env_2.py:616-637), every call's observation, reward and terminated kept.
 * actions_dev: int32 [K, N] on the device (row t * N + env), any int32 value (out of range = invalid action: reward -1.0, state unchanged).
 * rows_dev / row_stride_bytes: as bg_rollout_rows (16-byte aligned, stride a multiple of 16, >= BG_ROW_BYTES; 384 = whole lines).
 * rows_stride_steps != 0: record of step t of env e at row t * N + e ([K, N] records); 0: row e, overwritten every step.
 * The record is bg_rollout_rows': the 31 observation keys at the BG_ROW_* offsets plus the step's reward (f64), action (i32: the caller's value as
 * given) and terminated byte.  There are NO per-step truncated / info arrays on this path: callers who need them keep bg_step_many.
 * stats_dev: optional, as bg_rollout_rows (t0 = 0 at the call's first step).
 * Auto-reset follows the HANDLE's BG_FLAG_AUTORESET (as bg_step / bg_step_many do), not "always on" as the rollouts.  With bg_set_gather_peers the
 * call's last step lands in the gather buffers as after bg_rollout_rows.  BG_ENGINE=1 handles run it on bg_engine.h: same records. */
int bg_step_many_rows(bg_handle* h, int K, const int32_t* actions_dev, uint8_t* rows_dev, uint64_t row_stride_bytes,
                      int rows_stride_steps, bg_rollout_stats* stats_dev, void* stream);

/* bg_step_many_rows under SafeBalatroEnv's episode limits, inside the launch (bg_engine3.h's SAFE instantiation; the rule is csrc/bg_safe.h).
 * Replaces: `SafeBalatroEnv(env, max_invalid_actions=50, max_episode_steps=1000)` around every env of the reference's training scripts
 * (train_balatro_fixed.py:228-277, :292; robust_training.py:35) and the reset SB3's VecEnv gives an env the wrapper ended.  Per step, in the
 * reference's order:
 *     episode_steps += 1
 *     if reward == -1.0 (exactly, float64) and not the env's own terminated:  consecutive_invalid += 1; at max_invalid_actions: kill, reward = -50.0
 *     else: consecutive_invalid = 0
 *     max_steps = episode_steps >= max_episode_steps;  ended = env's terminated or kill or max_steps;  on `ended` both counters return to 0
 * (a failed consumable, BG_ERR_CONSUMABLE*, has reward -1.0 and counts as an invalid action, as in the reference).
 * limits == NULL: exactly bg_step_many_rows (byte BG_ROW_END_FLAGS stays 0).  With limits a record differs from bg_step_many_rows' in this:
 *   byte BG_ROW_TERMINATED is SB3's `done` = ended, with its documented meaning -- the step ended the episode, the record already shows the new one --
 *     so bg_gae_rows, bg_episode_stats_rows (Monitor sits outside SafeBalatroEnv) and bg_norm_reward_rows work on these records unchanged;
 *   byte BG_ROW_END_FLAGS holds the BG_END_* bits, non-zero exactly when byte BG_ROW_TERMINATED is set;
 *   a killed step's reward is -50.0 (every other reward is the step's own; the action word is the caller's value).
 * A wrapper-made ending -- kill or max_steps while the env itself did not terminate -- resets the env inside the same step as a game over does (the
 * same reset: templates re-applied, one ring deck consumed).  Before that reset the record as it stood -- SB3's info["terminal_observation"], with the
 * step's reward, action and ending bytes, terminated = 1 -- goes to terminal_rows[j * N + e] and terminal_step[j * N + e] = t, the step of THIS call,
 * where j counts the earlier wrapper endings of env e in this call: slots are per env, nothing is counted globally, two equal calls write equal
 * bytes.  The call sets every unused terminal_step entry to -1 and leaves unused terminal records untouched.  SB3 bootstraps where the flags are
 * exactly BG_END_MAX_STEPS (TimeLimit.truncated = truncated and not terminated).  stats_dev->episodes counts every ended episode.
 * BG_E_ARG (text "bg_step_many_rows_ex: ..." in bg_last_error(h)) before anything is launched: a limit below 3 (the look-ahead rings are sized on
 * episodes of at least 3 steps, which the game guarantees and such a limit would not), a handle without BG_FLAG_AUTORESET, a BG_ENGINE=1 handle,
 * misaligned counters or terminal buffers, a terminal stride that is no record stride, terminal_slots below bg_safe_terminal_slots, only one of the
 * two terminal pointers.  The counters are the caller's, like bg_episode_stats_rows' carries: zero them where bg_reset restarts an env. */
#define BG_ROW_END_FLAGS 343      /* uint8: why the step ended the episode (bg_step_many_rows_ex with limits; 0 on every other path) */
#define BG_END_GAME 1u            /* the env's own terminated (balatro_env_2.py:616-637, curriculum cap) */
#define BG_END_INVALID 2u         /* info['invalid_action_termination'] */
#define BG_END_MAX_STEPS 4u       /* info['max_steps_reached'] */
typedef struct bg_safe_limits {
  int32_t max_invalid_actions, max_episode_steps;  /* each >= 3 */
  int32_t* counters_dev;          /* int32 [N, 4], 16-byte aligned, in/out, caller-owned: episode_steps, consecutive_invalid, wrapper endings in
                                     this call (the library zeroes it at call start), 0 */
  uint8_t* terminal_rows_dev;     /* [S, N] records, or NULL */
  uint64_t terminal_stride_bytes; /* as row_stride_bytes */
  int32_t* terminal_step_dev;     /* int32 [S, N]: the step t of this call whose ending filled slot (j, e), else -1; NULL iff terminal_rows_dev is */
  int32_t terminal_slots;         /* S >= bg_safe_terminal_slots(K, limits) */
} bg_safe_limits;
/* K / min(limits) + 1: a call's first wrapper ending can come at its step 0 (the counters are carried in), each further one needs min(limits) more
 * steps.  BG_E_ARG for K < 0 or a limit below 3. */
int bg_safe_terminal_slots(int K, int max_invalid_actions, int max_episode_steps);
int bg_step_many_rows_ex(bg_handle* h, int K, const int32_t* actions_dev, uint8_t* rows_dev, uint64_t row_stride_bytes,
                         int rows_stride_steps, const bg_safe_limits* limits, bg_rollout_stats* stats_dev, void* stream);

/* bg_step_many_rows_ex with ProgressionRewardWrapper's reward shaping in front of the limits, inside the launch (bg_engine3.h's PROG instantiation; the
 * rule is csrc/bg_progress.h).
 * Replaces: `SafeBalatroEnv(ProgressionRewardWrapper(BalatroEnvFixed(seed + rank)), 50, 1000)` of train_progressive.py:123-131 (the wrapper:
 * train_progressive.py:21-120).  Per step, on the env's reward and on state.ante / state.round behind the step (the FINAL state's when the step ended
 * the game), in the reference's order, every addition one float64 rounding:
 *     total_steps += 1                                                                                   (:45)
 *     steps_on_current_ante = steps_on_current_ante + 1 if ante == last_ante else 0                      (:60-63)
 *     if ante > last_ante:  reward += 200 * (ante - last_ante); last_ante = ante                         (:66-72)
 *     if round > last_round and ante == last_ante:  reward += 20; last_round = round                     (:75-78)
 *     if ante > max_ante_reached:  max_ante_reached = ante; reward += 100                                (:81-86)
 *     if ante == 1 and steps_on_current_ante > 150:  reward += -0.5 * (steps_on_current_ante - 150)      (:91-93)
 *         if steps_on_current_ante > 300:  terminated = True ("stuck"); reward -= 50                     (:96-99)
 *     if total_steps > 200 and ante < 2: reward -= 0.2   elif total_steps > 400 and ante < 3: reward -= 0.3
 *                                                         elif total_steps > 600 and ante < 4: reward -= 0.4   (:103-108)
 *     if ante >= 3 and total_steps < 300:  reward += 50   (on every such step)                           (:111-114)
 *     if ante != last_ante:  last_round = round                                                          (:117-118)
 * and then SafeBalatroEnv's rule (above) on the SHAPED reward and on `the env's terminated or stuck`: an invalid action whose shaped reward is not
 * exactly -1.0 (-1.2 past step 200 on ante 1) is not counted, as in the reference; a stuck step zeroes consecutive_invalid like any terminated one.
 * The record's reward is the shaped one (-50.0 on a kill).  Byte BG_ROW_END_FLAGS: BG_END_STUCK when the wrapper ended the episode, BG_END_GAME only
 * for the env's own ending, BG_END_INVALID / BG_END_MAX_STEPS as above; a stuck step can carry BG_END_GAME or BG_END_MAX_STEPS too, and is never
 * bootstrapped (SB3 bootstraps only where the flags are exactly BG_END_MAX_STEPS).  A stuck ending the env did not make itself is a wrapper-made
 * ending like a kill: terminal record with the shaped reward to the env's next terminal slot, reset inside the step, the same accounting.  Every
 * ending returns the limits' counters and the progression carry to the reset state.  The episode summary (bg_set_episode_summary) works as with
 * bg_step_many_rows_ex: bytes 344..351 obey the switch; the rule reads the final ante and round whatever the switch says.
 * progress->counters_dev: int32 [N, 4], 16-byte aligned, in/out, caller-owned: total_steps, steps_on_current_ante,
 * (last_ante - 1) | (max_ante_reached - 1) << 16, last_round - 1 -- an all-zero row is the state after reset() (:33-41); zero it where bg_reset
 * restarts an env.  progress == NULL: exactly bg_step_many_rows_ex.
 * BG_E_ARG (text "bg_step_many_rows_progress: ..." in bg_last_error(h)) before anything is launched: progress without limits, a misaligned or missing
 * carry (or the limits' own counters passed as the carry), terminal_slots below bg_progress_terminal_slots, and everything bg_step_many_rows_ex
 * refuses (no auto-reset, BG_ENGINE=1, a limit below 3, ...). */
#define BG_END_STUCK 8u           /* info['stuck_on_ante_1'] (train_progressive.py:96-99) */
typedef struct bg_progress_rewards {
  int32_t* counters_dev;
} bg_progress_rewards;
/* K / min(max_invalid_actions, max_episode_steps, 301) + 1: a stuck ending needs 301 steps on ante 1.  BG_E_ARG for K < 0 or a limit below 3. */
int bg_progress_terminal_slots(int K, int max_invalid_actions, int max_episode_steps);
int bg_step_many_rows_progress(bg_handle* h, int K, const int32_t* actions_dev, uint8_t* rows_dev, uint64_t row_stride_bytes,
                               int rows_stride_steps, const bg_safe_limits* limits, const bg_progress_rewards* progress,
                               bg_rollout_stats* stats_dev, void* stream);

/* The ended episode's final ante, round and score in the record of the step that ended it: a switch of the handle, off by default.
 * Replaces: what the reference's callbacks log of every finished episode -- info's ante and chips_scored at `done` (train_balatro_agent.py:189-209)
 * -- and the `ante_at_end` CurriculumBalatroEnv's rule needs (train_balatro_agent.py:126-170), which SAME_STEP auto-reset overwrites before a
 * record is written.  With the switch on, every record of bg_step_many_rows_ex WITH limits whose byte BG_ROW_TERMINATED is set carries, in bytes
 * 344..351 (spare bytes inside BG_ROW_BYTES), the state the episode ended in -- the same whoever ended it: a game over, a curriculum cap (the end
 * ante is then cap + 1), an invalid-action kill or the step limit; every record whose terminated byte is 0 has zeros there.  Terminal records
 * (bg_safe_limits.terminal_rows_dev) are written before the reset: their observation IS the final state, and their bytes 344..351 stay 0.
 * With the switch on and limits == NULL, bg_step_many_rows_ex returns BG_E_ARG ("the episode summary needs limits").  bg_step_many_rows,
 * bg_rollout_rows, bg_step_rows and BG_ENGINE=1 never write the summary: their bytes 344..351 are 0 whatever the switch says.  The switch is handle
 * state, not part of a state blob (bg_get_state / bg_get_states).  Off: every byte the library writes is what it wrote before the switch existed.
 * enable: 0 or 1, BG_E_ARG otherwise. */
int bg_set_episode_summary(bg_handle* h, int enable);
#define BG_ROW_END_ANTE 344       /* int16: state.ante when the episode ended (>= 1) */
#define BG_ROW_END_ROUND 346      /* int8: state.round then; byte 347 stays 0 */
#define BG_ROW_END_CHIPS 348      /* uint32: min(chips_scored then, 2**32 - 1) */

/* Sharded jobs (one process per GPU): the exchange of the design -- every rank sees the CURRENT record of every env -- without a collective
 * behind the launch.  bufs[r] is rank r's gather buffer, uint8 [world][N][BG_ROW_BYTES], as mapped into THIS process (own buffer: an ordinary device
 * pointer; peers': hipIpcOpenMemHandle / torch's CUDA IPC over xGMI); N = this handle's env count, the same on every rank.  From then on the LAST launch
 * of every bg_rollout_rows call also writes the record of its last step into slot [rank] of all `world` buffers, from the engine's copy-out, while the
 * launch runs: when every rank's call has completed (a barrier between the ranks), every buffer holds all world x N current records.  world = 0 switches
 * it off.  Replaces: SubprocVecEnv's pipe traffic of observations to the learner process (hpc_train.py:60-65); the RCCL all_gather of
 * balatro_gym_amd/sharded.py stays as the fallback where peer mapping is not available. */
int bg_set_gather_peers(bg_handle* h, void* const* bufs, int world, int rank);

/* Harness injection (configs 3-4): per-env "reset template" applied by every reset of that env -- owned jokers (ids
 * from jokers.py), money, ante and hand levels; -1 / NULL leaves a field at its reset default.  apply_now != 0 also
 * writes them into the live state.  Replaces direct writes to env.state.* (e.g. train_balatro_agent.py:150). */
int bg_inject(bg_handle* h, const int32_t* jokers_host /*[N,5] or NULL*/, const int32_t* njokers_host /*[N]*/,
              const int64_t* money_host /*[N] or NULL*/, const int32_t* ante_host /*[N] or NULL*/,
              const uint8_t* levels_host /*[N,12] or NULL*/, const uint8_t* mask_host, int apply_now, void* stream);

/* The LIVE deck order of the masked envs: decks_host is [N, 52] card codes (rank-2)*4+suit, each row a permutation of 0..51.
 * Replaces direct writes to env.state.deck / env.game.deck (one aliased list, balatro_env_2.py:528-531), which is how a harness
 * or a test puts chosen cards under the hand's deck indexes (e.g. a straight flush at deck[0..4]: classification reads
 * deck[position]).  The next reset() reshuffles as always. */
int bg_inject_deck(bg_handle* h, const uint8_t* decks_host /*[N,52]*/, const uint8_t* mask_host, void* stream);

/* Card states (cards.py:62-139 CardState; the reference sets them through tarot cards -- not on this path -- the harness
 * injects them directly, like env.card_states[idx] = CardState(...)): per env and deck INDEX (position in the shuffled
 * deck, 0..51) the enhancement (0 none, 1 BONUS, 2 MULT, 3 WILD, 4 GLASS, 5 STEEL, 6 STONE, 7 GOLD, 8 LUCKY), edition
 * (0 none, 1 FOIL, 2 HOLOGRAPHIC, 3 POLYCHROME) and seal (0 none, 1 GOLD, 2 RED, 3 BLUE, 4 PURPLE) codes, [N, 52] u8 each
 * (NULL = all 0).  Effects on the path: balatro_env_2.py:287-325 (chips, stone), :703-767 (glass / lucky rolls on stream
 * 'card_enhancement', seals, steel, retriggers), :1334-1343 (gold).  reset() clears the states (:511); the injected set
 * is re-applied after every reset, like bg_inject's template.  Needs BG_FLAG_CARD_STATES at bg_create. */
int bg_inject_cards(bg_handle* h, const uint8_t* enh_host, const uint8_t* edition_host, const uint8_t* seal_host,
                    const uint8_t* mask_host, int apply_now, void* stream);

/* Consumables (balatro_env_2.py:1066-1172 _use_consumable over consumables.py; BASELINE config 4): per-env reset template
 * of state.consumables, ids as in _get_consumable_ids (balatro_env_2.py:1545-1567): tarots 1-22, planets 30-41,
 * spectrals 50-67; ids_host is [N, 2], n_host[i] in [0, 2] (-1 = back to the reset default).  Re-applied after every
 * reset like bg_inject's template.  Tarot / spectral cards edit card states, so they need BG_FLAG_CARD_STATES (planets do
 * not).  In-env sources of consumables: blue seals (planets), purple seals (tarots), The Fool / High Priestess /
 * Emperor / Judgement.  All 52 ids are followed (incl. the reference's quirks: INTEGRATION.md section 6); error codes
 * BG_ERR_CONSUMABLE / _RAISES / _DECK.  Replaces direct writes to env.state.consumables. */
int bg_inject_consumables(bg_handle* h, const int32_t* ids_host /*[N,2]*/, const int32_t* n_host /*[N]*/,
                          const uint8_t* mask_host, int apply_now, void* stream);

/* Replaces: save_state()/load_state() (balatro_env_2.py:1575-1615).  Blob = versioned raw copy of one env's state
 * (game + all RNG streams + look-ahead rings).  bg_state_blob_bytes gives the size. */
uint64_t bg_state_blob_bytes(const bg_handle* h);
int bg_get_state(bg_handle* h, int env_index, void* blob_host, uint64_t blob_bytes);
int bg_set_state(bg_handle* h, int env_index, const void* blob_host, uint64_t blob_bytes);

/* The same for MANY envs at once, the blobs staying on the device: one kernel launch (csrc/bg_snapshot.h) moves every slice of all m envs, 16 bytes
 * per lane wherever the piece allows.  Replaces: a loop of save_state() / load_state() over the envs of a SubprocVecEnv -- a checkpoint of the whole job
 * beside the normaliser's, or the N envs as branches of a search (fork one env into 60 and step each with another action: an exact one-step look-ahead).
 * The caller's EpisodeLimits / EpisodeStats / RowNormalizer carries are not part of a blob.
 *
 * Blobs: blob i starts at blobs_dev + i * blob_stride_bytes; blobs_dev is 16-byte aligned, the stride a multiple of 16 and at least
 * bg_state_blob_bytes(h); the bytes of a slot beyond the blob size are never written.  Index lists are int32 on the HOST and are copied before the
 * call returns.  All three are queued on `stream` like a step: they issue the pending pieces of a sliced refill and make `stream` wait for the handle's
 * latest refill with an EVENT (no device synchronisation); work of the handles that the caller put on OTHER streams is the caller's to order.
 *
 * bg_get_states: blob i = byte for byte what bg_get_state(h, env_index[i], ...) returns at that point of the stream, header included
 *   (env_index_host NULL = envs 0..m-1; repeated indices are allowed).  Does not wait for the host.
 * bg_set_states: env env_index[i] ends up exactly as bg_set_state(h, env_index[i], blob blob_index[i]) leaves it (blob_index_host NULL = blob i): the
 *   device state, both producer-counter buffers, the host mirrors of the reset template and the curriculum cap, and the handle counts as seeded.  One
 *   blob may go to many envs; env_index must be distinct.  The headers of all referenced blobs (magic, version, ring depths, card-state flag) are
 *   checked before anything is written: they are read back, with the template and cap words the mirrors need (64 bytes per pair, one copy), which
 *   SYNCHRONISES `stream` with the host.  The rings are topped up before the next step (as after bg_set_state).
 * bg_copy_states: env src_index[i] of `src` -> env dst_index[i] of `dst`, no blob in between.  dst == src (one handle) is allowed, and so is another
 *   handle on the same device with the same ring depths (KG / KS / KD) and card-state flag.  dst_index must be distinct; on one handle no dst may be the
 *   src of another pair, and a pair with dst == src moves nothing.  The host mirrors are copied mirror to mirror: no read-back, the call does not wait for
 *   the device -- the one a search loop calls every step.  Across handles the rings of `dst` are topped up before its next step; inside one handle
 *   the handle's own refill schedule already covers the copies (a dst's rings are exactly as deep as its src's: DESIGN.md section 3, "Many envs at once").
 *
 * BG_E_ARG, text "bg_get_states: ..." / "bg_set_states: ..." / "bg_copy_states: ..." in bg_last_error(h) (of `dst` for a copy), nothing written: an index
 * out of range, a repeated dst, dst / src overlap, m < 0, a null pointer, a misaligned base, a stride too small or no multiple of 16, a blob_index outside
 * [0, n_blobs), a bad header, handles on different devices or of different depths.  m == 0 is a no-op. */
int bg_get_states(bg_handle* h, const int32_t* env_index_host /*[m] or NULL = 0..m-1*/, int m, void* blobs_dev, uint64_t blob_stride_bytes, void* stream);
int bg_set_states(bg_handle* h, const int32_t* env_index_host /*[m]*/, int m, const void* blobs_dev, uint64_t blob_stride_bytes, int n_blobs,
                  const int32_t* blob_index_host /*[m] or NULL = i*/, void* stream);
int bg_copy_states(bg_handle* dst, const int32_t* dst_index_host, bg_handle* src, const int32_t* src_index_host, int m, void* stream);

/* Top up the RNG look-ahead rings (pre-shuffled decks, pre-seeded shop streams, global-stream blocks).  bg_step /
 * bg_reset / bg_rollout call it themselves; exposed for tests and for overlapping it on a side stream. */
int bg_refill(bg_handle* h, void* stream);

/* Measurement hooks (bench.py): when enabled every kernel launch is bracketed by HIP events on its own stream.
 * bg_get_profile synchronises and returns out8 = {rollout kernel ms, rollout launches, fused steps summed over
 * launches, refill kernel ms, refill launches, step kernel ms, step launches, 0} since the last call. */
int bg_set_profiling(bg_handle* h, int enable);
int bg_get_profile(bg_handle* h, double* out8);

/* Measurement hook (bench.py `roofline.peak_measured`): a plain streaming copy of `bytes` (16 B per lane, src -> dst, both
 * 16-byte aligned device buffers) repeated `iters` times; *gbps_out = (bytes read + bytes written) / time.  SURVEY 8(d): the
 * roofline fraction is quoted against the nominal 8 TB/s AND against what a copy kernel reaches on the same GPU. */
int bg_bench_copy(const void* src_dev, void* dst_dev, uint64_t bytes, int iters, double* gbps_out, void* stream);
/* The write-only twin (bench.py `roofline.peak_measured_write`): a plain fill of `bytes` (16 B per lane), *gbps_out = bytes written /
 * time.  The step path's algorithmic traffic is ~80 % stores (every step's record), so this is the ceiling that applies to it. */
int bg_bench_fill(void* dst_dev, uint64_t bytes, int iters, double* gbps_out, void* stream);

/* Check the sticky device error word (synchronises the stream). */
int bg_check(bg_handle* h, void* stream);

/* ---- Operator-level entry points: the units the reference exposes as callables of their own, batched (lane = case).  They
 * need no handle: they run on the CURRENT device, on caller-owned device buffers, and call the same device functions as the
 * step path.  bg_last_error(NULL) gives the text of a failure. ---- */

/* Replaces: `BalatroGame._classify_hand(cards)` (balatro_game.py:40-93).  cards_dev is [M, 8] card codes (rank-2)*4+suit
 * (8-byte aligned), n_dev[i] in [0, 8] of them are valid; hand_type_dev[i] = HandType value 0..8 (scoring_engine.py:12-24). */
int bg_classify_batch(const uint8_t* cards_dev, const uint8_t* n_dev, uint8_t* hand_type_dev, int64_t m, void* stream);
/* The same with the lane mapping chosen by the caller: lanes_per_case = 1 (lane = hand, the default above) or 8 (lane = card, the
 * counts and sets by `__shfl_xor` inside 8-lane groups -- the mapping SURVEY 7.6 asks to benchmark beside the first).  Results are
 * identical.  kernel_ms_out (may be NULL): time of the kernel alone, HIP events on `stream`; non-NULL synchronises the stream. */
int bg_classify_batch_ex(const uint8_t* cards_dev, const uint8_t* n_dev, uint8_t* hand_type_dev, int64_t m, int lanes_per_case,
                         float* kernel_ms_out, void* stream);

/* Replaces: `UnifiedScorer.score_hand(ctx)` (unified_scoring.py:111-299) called with game_state['jokers'] = joker NAMES (as
 * unified_scoring.py:313-351 does) after random.seed(gseed).  One int32[BG_SCORE_CASE_WORDS] record per case:
 *   [0..23] 8 x (rank 2..14 | 0 for a STONE card, suit 0..3 = C D H S | 4 = 'Stone', chip_value()) = context.cards
 *   [24] len(cards)  [25] the first nscoring of them are context.scoring_cards  [26] hand type 0..11
 *   [27] name style: 0 = balatro_env_2.py:674 ('One Pair', 'Three Kind', 'Four Kind'), 1 = balatro_sim ('Pair', ...)
 *   [28] hand level  [29] number of jokers  [30..34] joker ids (jokers.py)  [35] hands_left  [36] discards_left
 *   [37] len(game_state['deck'])  [38] gseed (< 2**32)  [39] 0
 * and one int64[BG_SCORE_OUT_WORDS] result: score, final chips, final mult, bits of the float64 x_mult, money gained, words
 * of the global stream consumed, the word the NEXT getrandbits(32) would return (identifies the stream position), 0 (word 7 is
 * always written, as 0).  Synchronises the stream. */
#define BG_SCORE_CASE_WORDS 40
#define BG_SCORE_OUT_WORDS 8
int bg_score_hand_batch(const int32_t* cases_dev, int64_t* out_dev, int m, void* stream);
/* The same with lanes_per_case = 1 or 8 (8: lane = card while the hand is gathered, lane = joker for the per-card joker phase whose
 * totals are shuffle reductions, lane = card for Bloodstone's RNG words; the order-dependent main phase runs on every lane).
 * kernel_ms_out (may be NULL): time of the scoring kernel alone (the per-case random.seed() runs in a kernel of its own before it). */
int bg_score_hand_batch_ex(const int32_t* cases_dev, int64_t* out_dev, int m, int lanes_per_case, float* kernel_ms_out, void* stream);

/* balatro_sim.py (the reference's secondary, Balatro-accurate evaluator / scorer; not reachable from the live env).  A sim card
 * is six int32: rank 2..14, suit 0..3 = Clubs, Diamonds, Hearts, Spades, base_value, enhancement (0 None, 1 'bonus', 2 'mult',
 * 3 'wild', 4 'glass', 5 'steel', 6 'stone', 7 'gold', 8 'lucky'), edition (0 None, 1 'foil', 2 'holographic', 3 'polychrome',
 * 4 'negative'), seal (0 None, 1 'gold', 2 'red', 3 'blue', 4 'purple').  Hand types 0..11 = High Card, Pair, Two Pair, Three
 * of a Kind, Straight, Flush, Full House, Four of a Kind, Straight Flush, Five of a Kind, Flush House, Flush Five.
 *
 * Replaces: `BalatroSimulator.evaluate_hand(cards)` (balatro_sim.py:220-366 over get_x_same :108-126, get_flush :128-149,
 * get_straight :151-214).  hands_dev is int32 [M, 8, 6], n_dev[i] in [0, 8] cards are valid, flags_dev[i] bit 0 = a Four Fingers
 * joker is owned, bit 1 = Shortcut.  out_dev is int8 [M, BG_SIM_EVAL_BYTES]: [0] results['top']; [1..12] len(results[type]);
 * [13..24] len(results[type][0]); [32 + 8 * type + k] = position in the hand of card k of results[type][0] (-1 padded).
 * Bytes 25..31 of a row are not written: they keep what the caller's buffer held. */
#define BG_SIM_EVAL_BYTES 128
int bg_sim_evaluate_batch(const int32_t* hands_dev, const int32_t* n_dev, const int32_t* flags_dev, int8_t* out_dev, int m, void* stream);

/* Replaces: `BalatroSimulator.calculate_score(cards, game_state)` (balatro_sim.py:402-548) after random.seed(seed).  One
 * int32[BG_SIM_CASE_WORDS] record per case: [0..47] 8 sim cards, [48] number of cards, [49] number of jokers,
 * [50..54] player_state.jokers (ids; Four Fingers 18 / Shortcut 69 act on the evaluation and draw like any other joker),
 * [55] game_state['hands_left'] (1 when the key is absent, complete_joker_effects.py:46), [56] 'discards_left' (0 when absent),
 * [57] len(game_state['deck']), [58] seed (< 2**32), rest 0.  Result int64[8]: score, chips, added mult, bits of the float64
 * x_mult, money gained, words of the global stream consumed, the word the next getrandbits(32) returns, top | nscoring << 8.
 * Synchronises the stream. */
#define BG_SIM_CASE_WORDS 64
int bg_sim_score_batch(const int32_t* cases_dev, int64_t* out_dev, int m, void* stream);

/* Packed records -> the float matrix a policy network reads, in ONE launch: the consumer of bg_rollout_rows / bg_step_rows /
 * bg_step_many_rows.  Replaces the host glue between the env and the network's first layer:
 *   BG_ENC_PRODUCED / BG_ENC_FIXED  SB3's `CombinedExtractor` under `MultiInputPolicy` over `BalatroEnvFixed` (hpc_train.py:77,
 *     train_balatro_fixed.py:125-207,346): every key flattened, `.float()`ed and concatenated in the observation space's key order.
 *     PRODUCED: the 31 keys `_get_observation()` fills (balatro_env_2.py:1488-1531; the order of bg_obs_ptrs), every element as
 *     numpy.float32(value) -- round to nearest even above 2**24, `chips_scored` straight from int64 (`_fix_observation` does not narrow
 *     it), `progress_ratio` bit for bit: 153 columns.  FIXED: PRODUCED followed by the 20 keys the env declares (balatro_env_2.py:386-470)
 *     and never fills, which BalatroEnvFixed zero-fills: 475 zeros, 628 columns; its first 153 columns are PRODUCED.
 *   BG_ENC_EXTRACTOR  the tensors `BalatroFeaturesExtractor.forward` builds (train_balatro_agent.py:84-119): columns [0, 416) the hand
 *     one-hot, column slot * 52 + card = 1.0 where hand[slot] == card (:86-93; defined for hand values -1..51, what the env writes: the -1
 *     padding sets nothing); [416, 426) `joker_ids.float()` (:98); [426, 447) chips_scored / 1e6, chips_needed / 1e5, progress_ratio,
 *     money / 100, ante / 10, round / 3, hands_left / 10, discards_left / 5, hand_levels[0..11] / 10, phase / 3 (:102-113), each
 *     numpy.float32(value) / numpy.float32(c): an IEEE float32 division, not a multiplication by a reciprocal.  (The reference's
 *     constructor sizes its game-state layer for 32 inputs while its forward builds these 21: size a first layer from bg_encode_cols.)
 * out_dtype BG_ENC_BF16: the float32 value rounded to nearest even (`tensor.to(torch.bfloat16)`; a NaN becomes 0x7fc0).
 * rows_dev: m records as the row paths write them (16-byte aligned, row_stride_bytes a multiple of 16, >= BG_ROW_BYTES; a [K, N, stride]
 * buffer is m = K * N).  out_dev: [m, out_stride_elems] elements of out_dtype (aligned to its element), out_stride_elems >= the column
 * count; columns beyond the count are left untouched.  16-byte stores when out_dev and the row pitch are 16-byte aligned, or when out_dev
 * is and the matrix is dense (out_stride_elems == columns); one element per lane otherwise.  The record's reward / action / terminated are
 * in no layout.  kernel_ms_out as in bg_classify_batch_ex.  Runs on the current device; bg_last_error(NULL) has the text of a BG_E_ARG;
 * m == 0 is a no-op. */
#define BG_ENC_PRODUCED 0
#define BG_ENC_FIXED 1
#define BG_ENC_EXTRACTOR 2
#define BG_ENC_F32 0
#define BG_ENC_BF16 1
int bg_encode_cols(int layout); /* number of columns, or BG_E_ARG */
int bg_encode_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t m, int layout, int out_dtype,
                   void* out_dev, uint64_t out_stride_elems, float* kernel_ms_out, void* stream);

/* PPO's two scans along K over a finished [K, N] rollout of packed records, on the device, in ONE launch each: the consumers of
 * bg_rollout_rows / bg_step_many_rows beside bg_encode_rows.  Both read two fields of a record, BG_ROW_REWARD and BG_ROW_TERMINATED.
 * Record (t, e) is at rows_dev + (t * N + e) * row_stride_bytes (the rows_stride_steps != 0 layout; a RowBuffers.rows tensor); rows_dev 16-byte
 * aligned, row_stride_bytes a multiple of 16 and >= BG_ROW_BYTES.  Both run on the current device, need no handle, return BG_E_ARG (text in
 * bg_last_error(NULL)) before launching anything, treat K == 0 or N == 0 as a no-op; kernel_ms_out as in bg_classify_batch_ex.
 *
 * bg_gae_rows replaces: SB3's `RolloutBuffer.compute_returns_and_advantage`, which every training script of the reference runs through
 * `PPO(..., gamma=0.99, gae_lambda=0.95)` (hpc_train.py:77-86, train_balatro_fixed.py:346-355, train_balatro_agent.py:329-335,
 * train_progressive.py:164-171, robust_training.py:143-149): a loop over the K steps, backwards, a handful of elementwise operations per step.
 * The result is, bit for bit, that loop run in numpy on float32 buffers, with episode_starts[t + 1] = dones[t] = the record's terminated byte of
 * step t (SAME_STEP auto-reset: the record of a terminated step already shows the next episode, so values[t + 1] belongs to it and is cut off):
 *     g = float32(gamma);  gl = float32(gamma * gae_lambda)   (the product taken in float64 first);  last = 0
 *     for t = K-1 .. 0:  r = float32(reward[t])  (round to nearest even);  nnt = 1 - float32(terminated[t] != 0)
 *                        nv = t == K-1 ? last_values[e] : values[t+1][e]
 *                        delta = (r + (g * nv) * nnt) - values[t][e];  last = delta + ((gl * nnt) * last)
 *                        advantages[t][e] = last;  returns[t][e] = last + values[t][e]
 * every operation rounded to float32, no fused multiply-add.  values_dev / advantages_dev / returns_dev are dense float32 [K, N], last_values_dev
 * [N]; returns_dev may be NULL (not written).  Outputs must not alias inputs or each other.  A truncation bootstrap is the caller's addition to the
 * rewards (bg_gae_rows_ex's rewards_dev): records of bg_step_many_rows_ex say in byte BG_ROW_END_FLAGS where the step limit alone ended an episode.
 *
 * bg_episode_stats_rows replaces: `Monitor` (hpc_train.py:26, train_balatro_fixed.py:290), the source of ep_rew_mean / ep_len_mean, as
 * info['episode']['r' / 'l'].  Per env, forwards: carry_return += reward[t] (a plain float64 sum in step order), carry_len += 1; on a set
 * terminated byte ep_return[t][e] / ep_len[t][e] = the carries and the carries return to 0.0 / 0, otherwise the outputs are written as 0.0 / 0.
 * The carries ([N], in / out) hold the running episode after the call, so 2 K steps give the same outputs in two calls of K as in one.  Monitor's own
 * presentation (round(..., 6), CPython's compensated sum) is not promised to the last bit.  ep_return_dev / ep_len_dev: dense [K, N], each may be NULL;
 * they must not alias the carries.  Wrapper-made endings (SafeBalatroEnv's invalid-action / step limits) are in the records of bg_step_many_rows_ex
 * (terminated byte set, reward -50.0 on a kill: what Monitor, which sits outside SafeBalatroEnv, sees); no other rows call makes them. */
int bg_gae_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N,
                const float* values_dev, const float* last_values_dev, double gamma, double gae_lambda,
                float* advantages_dev, float* returns_dev, float* kernel_ms_out, void* stream);
int bg_episode_stats_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N,
                          double* ep_return_carry_dev, int32_t* ep_len_carry_dev, double* ep_return_dev, int32_t* ep_len_dev,
                          float* kernel_ms_out, void* stream);

/* bg_gae_rows with the rewards taken from a dense float64 [K, N] array instead of the records (rewards_dev; NULL = the record's reward: then it IS
 * bg_gae_rows): how the normalised rewards of bg_norm_reward_rows reach the advantage scan.  Each value is converted to float32 as the record's reward
 * is (round to nearest even); the terminated byte still comes from the record.  rewards_dev is 8-byte aligned and must not alias an output. */
int bg_gae_rows_ex(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N,
                   const float* values_dev, const float* last_values_dev, double gamma, double gae_lambda,
                   float* advantages_dev, float* returns_dev, const double* rewards_dev, float* kernel_ms_out, void* stream);

/* The ended episodes of a finished [K, N] rollout of packed records, in ONE launch (csrc/bg_ends.h): a report for logging and, optionally, the
 * curriculum's cap updates, on the device.  Reads the last 16 bytes of every record (336..351: the terminated byte, BG_ROW_END_FLAGS and the episode
 * summary of bg_set_episode_summary), i.e. one 128-byte line per record.  Record layout, alignment, BG_E_ARG (text in bg_last_error(NULL)) before
 * anything is launched, the current device and kernel_ms_out are as in bg_gae_rows; lane = env, forwards along K.
 * Replaces: the per-episode logging of the reference's callbacks (train_balatro_agent.py:189-209) and `CurriculumBalatroEnv` (:126-170), which
 * sb3_adapter.CurriculumTracker.update vectorises on the host.
 * report_dev: int64 [BG_ENDS_WORDS], 8-byte aligned, overwritten by every call (K * N == 0: zeros); integer sums, so two calls give equal values:
 *     0       records with byte BG_ROW_TERMINATED set ("ended records")
 *     1 2 3   of those: BG_ROW_END_FLAGS & BG_END_GAME, & BG_END_INVALID, == BG_END_MAX_STEPS
 *     4 5     sum and maximum of the end ante              6 7   sum and maximum of the end chips
 *     8       envs whose cap this call raised (0 without cur)
 *     9       ended records whose end ante is <= 0, i.e. made without the summary: they count in words 0..3 only and are not fed to the curriculum
 *     10..15  0
 *     16 + min(end ante, 15)   histogram of the end ante
 * cur (NULL: the report alone): per env, for every ended record with a summary in step order, CurriculumTracker.update's rule for that env:
 *     hist[count % window][e] = end ante;  count += 1;  at_level += 1
 *     if at_level >= window and (number of kept entries >= cap) / float64(window) >= threshold:  cap = min(cap + increment, 255);  at_level = 0
 * where the kept entries are the first `count` while count < window (the division is by `window` all the same, as in the reference); the float64
 * division and compare are done as written, so the decision is exact.  An env with cap 0 (no cap) keeps its history and is never raised.
 * A raised cap takes effect at the CALL BOUNDARY: the caller hands cap_dev to bg_set_max_ante behind the call (where word 8 is non-zero).  Episodes
 * the env finishes later in the same rollout were played under the old cap and enter the history as played, judged against the new cap.
 * cap_dev int32 [N] in / out; hist_dev int16 [window, N] in / out; count_dev int64 [N] in / out; at_level_dev int32 [N] in / out (saturates at
 * 2**31 - 1); raised_dev uint8 [N] out: 1 where this call raised the env's cap at least once, else 0.
 * BG_E_ARG: K < 0 or N < 0, rows_dev / row_stride_bytes that are no records, report_dev NULL or misaligned; with cur: a NULL or misaligned array,
 * window < 1, increment outside 1..255, a threshold that is not finite. */
#define BG_ENDS_WORDS 32
typedef struct bg_curriculum {
  int32_t* cap_dev;      /* [N] in/out, current_max_ante per env, 1..255; an env with cap 0 is never raised */
  int16_t* hist_dev;     /* [window, N] in/out: final antes of the last `window` episodes, slot count % window */
  int64_t* count_dev;    /* [N] in/out: episodes ever finished */
  int32_t* at_level_dev; /* [N] in/out: episodes since the env's last raise */
  uint8_t* raised_dev;   /* [N] out: 1 where this call raised the cap at least once */
  int32_t window, increment; double threshold;
} bg_curriculum;
int bg_episode_ends_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N,
                         int64_t* report_dev, const bg_curriculum* cur, float* kernel_ms_out, void* stream);

/* SB3's VecNormalize over [K, N] packed records, on the device: the last wrapper between the env and the network in the reference's training scripts.
 * Replaces: `VecNormalize(env, norm_obs=True, norm_reward=True, clip_obs=10.0)` (hpc_train.py:68,72; train_balatro_agent.py:319,323), whose pickle is
 * saved beside every checkpoint (hpc_train.py:101-107,151-152): per step a numpy mean / var over the envs of every key, a RunningMeanStd merge, a
 * subtract / divide / clip, and the same for the discounted-return statistics of the reward.
 * Records, K, N, alignment: as bg_gae_rows (record (t, e) at rows_dev + (t * N + e) * row_stride_bytes; 16-byte aligned; stride a multiple of 16, >=
 * BG_ROW_BYTES).  Both calls run on the current device, need no handle, return BG_E_ARG (text in bg_last_error(NULL)) before launching anything, treat
 * K == 0 or N == 0 as a no-op, never synchronise the host (several launches on `stream`); kernel_ms_out as in bg_classify_batch_ex.
 * workspace_dev: 16-byte aligned scratch of >= bg_norm_workspace_bytes(K, N) bytes (the per-workgroup partial moments of either call).
 *
 * RunningMeanStd (float64; a fresh one is mean 0, var 1, count 1e-4) is updated with a batch's mean bm, population variance bv and size n by
 *     delta = bm - mean;  tot = count + n;  new_mean = mean + delta * n / tot;  m_a = var * count;  m_b = bv * n
 *     m_2 = m_a + m_b + square(delta) * count * n / (count + n);  new_var = m_2 / (count + n);  new_count = n + count
 * evaluated left to right, every operation rounded on its own (no fused multiply-add), `/` and sqrt IEEE operations.
 *
 * bg_norm_obs_rows: step t is the batch of the N records (t, 0..N-1).  The statistics are one (mean, var) per column of the BG_ENC_PRODUCED layout
 * (153 columns: one RunningMeanStd per key, of the key's shape) and one shared count.  update != 0: per step, in order, the statistics are updated
 * with the step's batch moments and row t is normalised with the statistics AFTER its own update,
 *     out[t][e][c] = float32(clip((float64(x) - mean[c]) / sqrt(var[c] + epsilon), -clip_obs, clip_obs))
 * (x converted from the key's own dtype); after the call mean_dev / var_dev / count_dev hold the state behind step K-1.  update == 0: every row is
 * normalised with the statistics as given, which are not written; moments_dev must be NULL.  layout BG_ENC_PRODUCED or BG_ENC_FIXED (its columns
 * 153..627 are written as 0.0 and carry no statistics: (0 - 0) / sqrt(var + epsilon)); BG_ENC_EXTRACTOR is a BG_E_ARG.  out_dtype BG_ENC_BF16: the
 * float32 result rounded to nearest even.  out_dev: [K * N, out_stride_elems], columns beyond the layout's count left untouched, 16-byte stores
 * under bg_encode_rows' rule; NULL = statistics only.  moments_dev: [K, 2, 153], the batch mean and batch variance of every step, or NULL.
 *
 * bg_norm_reward_rows, per step t: ret[e] = ret[e] * gamma + reward[t][e]; ret_stats (mean, var, count of a RunningMeanStd of shape ()) is updated with
 * the batch moments of ret over e; rewards[t][e] = clip(reward[t][e] / sqrt(var + epsilon), -clip_reward, clip_reward) (float64, dense [K, N], may be
 * NULL); ret[e] = 0 where the record's terminated byte is set.  returns_carry_dev [N] holds ret across calls: 2 K steps give the same bits in two
 * calls of K as in one.  update == 0: only the normalisation, with ret_stats as given; neither ret_stats nor the carry is written.  moments_dev: [K, 2].
 *
 * What is numpy's to the bit and what is bounded: the batch moments are the mean and population variance of float64(x) over the N envs, reduced as
 * (n, mean, M2) triples merged in a fixed tree -- deterministic (no atomics; the same inputs give the same bits on every call), exactly 0.0 variance
 * for a column that is constant over the batch, and within summation error of numpy.mean / numpy.var(x.astype(float64), axis=0), whose own order of
 * additions is an implementation detail.  (For the float32 key `progress_ratio` this is more accurate than SB3, which sums that key in float32.)
 * Everything behind the reduction -- the merge chain, the normalisation, the return recurrence -- is bit for bit the float64 expressions above.
 * Outputs must not alias inputs or each other.  Truncation, the extractor layout and terminal observations are out of scope. */
#define BG_NORM_COLS 153
uint64_t bg_norm_workspace_bytes(int K, int64_t N);
int bg_norm_obs_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, int layout, int out_dtype,
                     double* mean_dev, double* var_dev, double* count_dev, int update, double epsilon, double clip_obs,
                     void* out_dev, uint64_t out_stride_elems, double* moments_dev,
                     void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);
int bg_norm_reward_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N,
                        double* returns_carry_dev, double* ret_stats_dev, int update, double gamma, double epsilon, double clip_reward,
                        double* rewards_dev, double* moments_dev,
                        void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);

/* One minibatch's network input straight from the stored records, in ONE launch: bg_encode_rows, or bg_norm_obs_rows with frozen statistics, for the
 * rows an index names.  The other half of bg_ppo_loss' index_dev: the logits that call consumes come from the features of the same rows index[i].
 * Replaces: SB3's `RolloutBuffer.get`, which `PPO.train` runs n_epochs (10 in hpc_train.py:77-86) times per rollout: `observations[key][indices]`
 * for every key of a random permutation's slice, on top of a rollout stored as floats.  Here the rollout stays the 352-byte records; neither the
 * [K * N, columns] feature matrix nor a gathered copy of the records exists.
 * rows_dev: store_rows records under bg_encode_rows' rules (16-byte aligned, row_stride_bytes a multiple of 16, >= BG_ROW_BYTES).  index_dev: int32
 * [m], 4-byte aligned -- the convention of bg_ppo_loss' index_dev / store_rows, so ONE tensor serves both calls (index t * N + e names record
 * (t, e)); output row i is made from record index_dev[i]; repeats are allowed; an index outside [0, store_rows) reads nothing and row i is written
 * as +0.0 in every column of the layout (bg_ppo_loss excludes and counts such a row).  index_dev == NULL: row i from record i, m <= store_rows.
 * mean_dev == var_dev == NULL: row i is, bit for bit, the row bg_encode_rows writes for that record alone (any layout).  Both given: double[153]
 * each, 8-byte aligned, the statistics of bg_norm_obs_rows; row i is, bit for bit, the row bg_norm_obs_rows(update = 0) writes for that record with
 * these statistics, epsilon and clip_obs (BG_ENC_FIXED's columns 153..627: 0.0); layout BG_ENC_PRODUCED or BG_ENC_FIXED.  The statistics are only
 * read; there is no count and no workspace.
 * out_dev, out_dtype, out_stride_elems, the untouched columns beyond the count, the 16-byte store rule, kernel_ms_out: as bg_encode_rows; rows at or
 * beyond m are not touched.  Runs on the current device, needs no handle, never synchronises the host unless kernel_ms_out is given; m == 0 is a
 * no-op.  BG_E_ARG (text "bg_encode_rows_ex: ..." in bg_last_error(NULL)) before anything is launched: a misaligned pointer, a stride below
 * BG_ROW_BYTES or no multiple of 16, out_stride_elems below the column count, an unknown layout or dtype, store_rows < 0, store_rows > INT32_MAX
 * with an index, m > store_rows without one, only one of mean_dev / var_dev, statistics with BG_ENC_EXTRACTOR, epsilon or clip_obs negative or not
 * finite when statistics are given, out_dev equal to an input pointer.
 * Out of scope: statistics updates over a minibatch (an update is defined per step over all N envs: bg_norm_obs_rows); the extractor layout with
 * statistics; int64 indices; a gathered bg_norm_reward_rows (normalised rewards are stored dense and bg_ppo_loss gathers what follows from them);
 * shifting an index from a step to the record before it -- a record's observation and mask belong to the NEXT action (the head's note on alignment
 * in time), and that bookkeeping stays with the caller. */
int bg_encode_rows_ex(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                      const int32_t* index_dev /*nullable*/, int64_t m, int layout, int out_dtype,
                      const double* mean_dev /*nullable*/, const double* var_dev /*nullable*/,
                      double epsilon, double clip_obs,
                      void* out_dev, uint64_t out_stride_elems, float* kernel_ms_out, void* stream);

/* The masked categorical policy head: [m, 60] logits -> the int32 actions bg_step_rows / bg_step_many_rows take, with the log-probability and the
 * entropy PPO stores, in ONE launch; bg_evaluate_actions is the forward pass for given actions.  The arithmetic is csrc/bg_head.h.
 * Replaces: with mask_dev == NULL, SB3's `CategoricalDistribution.sample / log_prob / entropy / mode` as `PPO("MultiInputPolicy", ...)` runs them on
 * every step (hpc_train.py:77-86); with a mask, the discipline of the reference's own driver loop, which draws only from `action_mask`
 * (balatro_env_2.py:1841-1849) -- an invalid action costs reward -1.0 and a wasted step (balatro_env_2.py:625-627), and the training scripts, which
 * ignore the mask, end an episode with -50 after 50 of them (SafeBalatroEnv, train_balatro_fixed.py:228-283).
 *
 * A row is 60 logits l[j] (BG_HEAD_F32, or BG_HEAD_BF16 widened exactly: bits << 16) and 60 mask bytes (non-zero = valid; mask_dev == NULL = all
 * valid); V = the valid j.  All arithmetic is float32, every operation rounded on its own (no fused multiply-add):
 *     m = max over V of l[j];  d[j] = l[j] - m;  e[j] = expf(d[j]);  P[j] = running sum of e over the valid j in index order 0..59;  S = P[59]
 *     A = running sum, same order, of e[j] * d[j] over the valid j with e[j] > 0
 *     sample:         h = bg_policy_hash(seed, index0 + i, t)  (the rollout's splitmix64 counter hash, high 32 bits);  u = float(h >> 8) * 2^-24;
 *                     action = the smallest valid j with P[j] > u * S  (else the largest valid j with e[j] > 0: never taken for finite inputs)
 *     deterministic:  action = the smallest valid j with l[j] == m                                                (flags & BG_HEAD_DETERMINISTIC)
 *     log_prob = d[action] - logf(S);  entropy = logf(S) - A / S
 *     evaluate:       the action is given; in range but masked -> log_prob = -inf; outside [0, 60) -> log_prob = NaN; the entropy is unchanged
 * A DEGENERATE row -- V empty, a valid logit NaN or +inf, or every valid logit -inf -- gives action = -1 (an invalid action to the step entry points)
 * and log_prob = entropy = quiet NaN (0x7fc00000) in every mode; a valid -inf logit beside finite ones has probability 0.  So a masked action and an
 * action of probability 0 are never returned, and row i is a pure function of (its logits, its mask, seed, index0 + i, t): independent of m, of the
 * launch shape and of sharding (index0 / t mirror bg_rollout's env_index0 / t0: a sharded job passes its shard's first global env).  expf / logf are the
 * device library's accurate functions: the same inputs give the same bits on every call; they are bounded against float64, not promised glibc's bits.
 *
 * logits_dev: row i starts at element i * logits_stride_elems (>= 60), the pointer aligned to the element.  mask_dev: the first row's 60 mask bytes,
 * row i at + i * mask_stride_bytes (>= 60, a multiple of 4), the pointer 4-byte aligned; the mask of records is rows_dev + BG_ROW_ACTION_MASK with
 * the row stride (offset 176 is 16-byte aligned), the per-key layout's [N, 60] int8 array passes stride 60.  16-byte loads when pointer and row
 * pitch are 16-byte aligned or the pointer is and the matrix is dense; 4- or 2-byte loads per lane otherwise.  ALIGNMENT IN TIME: a record's mask is
 * the mask AFTER that record's step, so it belongs to the NEXT action (record t's mask goes with the logits computed from record t).
 * actions_dev int32 [m]; log_prob_dev / entropy_dev float32 [m], each may be NULL.  Outputs must not alias inputs or each other.  Both calls run on the
 * current device, need no handle, return BG_E_ARG (text in bg_last_error(NULL)) before launching anything, treat m == 0 as a no-op and never
 * synchronise unless timing is asked for; kernel_ms_out as in bg_classify_batch_ex.  Both are forward passes: the gradient through this head is bg_ppo_loss
 * (below).  Temperature and truncation are out of scope. */
#define BG_HEAD_F32 0
#define BG_HEAD_BF16 1
#define BG_HEAD_DETERMINISTIC 1u /* flags */
int bg_sample_actions(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems,
                      const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m, uint32_t flags,
                      uint64_t seed, uint64_t index0, uint64_t t,
                      int32_t* actions_dev, float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
                      float* kernel_ms_out, void* stream);
int bg_evaluate_actions(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems,
                        const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m,
                        const int32_t* actions_dev, float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
                        float* kernel_ms_out, void* stream);

/* PPO's clipped loss over the masked head above, its diagnostics, and its gradient with respect to the logits and the values, in one pass over the
 * logits: what a learner needs to train through the head that collected its data.  The arithmetic and the order of every operation are csrc/bg_ppo.h.
 * Replaces: the loss of SB3's `PPO.train` (masked_fill -> log_softmax -> gather -> exp -> clamp -> min -> mean, the entropy and value terms) and its
 * autograd backward, which every training script of the reference runs n_epochs = 10 times over each rollout (hpc_train.py:77-88,
 * train_balatro_fixed.py:346-357, train_balatro_agent.py:326-337, robust_training.py:140-151: clip_range 0.2, ent_coef 0.01, vf_coef 0.5;
 * train_progressive.py:161-176: 0.3 / 0.02).
 *
 * Row i of the minibatch reads its logits and value at i.  With index_dev (SB3's RolloutBuffer.get permutation, int32 [m]) the STORED arrays -- mask,
 * actions, old_log_prob, advantages, returns -- are read at row index[i] of store_rows rows, so the minibatch is gathered inside the launch and a
 * record's mask is read in place (rows_dev + BG_ROW_ACTION_MASK, the row stride); without it they are read at i.  All arithmetic is float32, every
 * operation rounded on its own; the sums across rows are float64.  m_, d[j], e[j], S, A, logS are bg_head_row's, so log_prob and entropy H are bit for
 * bit what bg_evaluate_actions returns for the row.
 *     adv'  = adv, or with BG_PPO_NORMALIZE_ADV and n > 1: (adv - mean) / (std + 1e-8f); mean / std: float64 mean and unbiased standard deviation of the
 *             call's n advantages (n = m less the rows whose index is out of range), rounded to float32 -- SB3's rule, its `len > 1` included
 *     lr = log_prob - old_log_prob;  ratio = expf(lr);  lo = 1 - clip;  hi = 1 + clip;  rc = min(max(ratio, lo), hi);  s1 = adv' * ratio;  s2 = adv' * rc
 *     policy term = -min(s1, s2);  g = adv' * ratio if (lo <= ratio <= hi) or s1 < s2, else 0   (torch's min / clamp backward, ties included)
 *     kl term = (ratio - 1) - lr;  clipped = |ratio - 1| > clip
 *     with values_dev / returns_dev (both or neither):  dv = v - ret;  value term = dv * dv;  dvalues[i] = ((vf_coef * 2) * dv) / float(m)
 *     p = e[j] / S;  valid j with e[j] > 0:  dlogits[i, j] = ((ent_coef * p) * ((d[j] - logS) + H) - g * (1[j == a] - p)) / float(m)
 *     valid j with e[j] == 0: (0 - g) / float(m) if j == a, else +0.0;  invalid j: +0.0;  padding columns of a strided dlogits are not written
 *     policy_loss = sum policy / m;  value_loss = sum value / m;  entropy_loss = -(sum H) / m;  approx_kl = sum kl / m;  clip_fraction = sum clipped / m
 *     loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss        (float64 from the float64 sums, each scalar rounded to float32 once)
 * An EXCLUDED row -- degenerate for the head, action outside [0, 60) or masked, old_log_prob / adv / adv' / value / return not finite, index outside
 * [0, store_rows) (nothing is read for it; log_prob = entropy = quiet NaN) -- adds nothing to any sum, has dlogits row and dvalue +0.0, is counted, and
 * the divisor stays m.  The sums take a fixed order (64 rows per workgroup by a tree, the workgroups' partials from workspace_dev in index order by
 * slices and a tree, in a one-workgroup kernel; no floating-point atomics), so two calls give the same bits.
 * stats_dev, float32 [BG_PPO_STATS]: loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv_mean, adv_std (0 without the flag),
 * excluded rows, m.  dlogits_dev has the dtype of the logits (bfloat16: the float32 value rounded to nearest even) and its own row stride (>= 60).
 * dvalues_dev, log_prob_dev, entropy_dev may be NULL.  Alignment rules and load paths as above; the gradient tile leaves by the mirror of those paths
 * (16-byte pieces, words or halves by the alignment of dlogits_dev).  workspace_dev: 16-byte aligned, bg_ppo_loss_workspace_bytes(m) bytes.
 * BG_E_ARG (text "bg_ppo_loss: ..." in bg_last_error(NULL)) before anything is launched for: wrong alignment, a stride < 60, an output that is the same
 * pointer as an input or another output, values without returns, clip_range outside (0, 1), a non-finite coefficient, a workspace too small, unknown
 * flags.  m == 0 writes zeros to stats_dev and launches nothing else.  Never synchronises unless timing is asked for.
 * Out of scope: clip_range_vf, temperature, target_kl early stopping (read approx_kl), gradient clipping, the optimiser. */
#define BG_PPO_STATS 10
#define BG_PPO_NORMALIZE_ADV 1u /* flags */
uint64_t bg_ppo_loss_workspace_bytes(int64_t m);
int bg_ppo_loss(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems,
                const int8_t* mask_dev /*nullable*/, uint64_t mask_stride_bytes,
                const int32_t* actions_dev, const float* old_log_prob_dev, const float* advantages_dev,
                const float* values_dev /*nullable*/, const float* returns_dev /*nullable*/,
                const int32_t* index_dev /*nullable*/, int64_t store_rows, int64_t m,
                float clip_range, float ent_coef, float vf_coef, uint32_t flags,
                void* dlogits_dev, uint64_t dlogits_stride_elems, float* dvalues_dev /*nullable*/,
                float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
                float* stats_dev /* float32[BG_PPO_STATS = 10] */,
                void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);

/* Behaviour cloning on records, in two stateless calls on caller-owned buffers.  Replaces: `BehavioralCloning` (train_balatro_agent.py:220-262),
 * reached through the script's `expert_trajectories=` argument: it keeps only the steps of trajectories with final_ante >= 5 ("only use successful
 * trajectories") and stops at `# TODO: Implement actual BC training loop`.
 *
 * bg_episode_outcome_rows (csrc/bg_outcome.h): ONE launch gives every step of a finished [K, N] rollout the outcome of its OWN episode -- the filter
 * above, the Monte-Carlo return of a step, and the distance to the episode's end.  Records, K, N, alignment, the current device, BG_E_ARG (text
 * "bg_episode_outcome_rows: ..." in bg_last_error(NULL)) before anything is launched, K == 0 or N == 0 a no-op and kernel_ms_out: as bg_gae_rows.
 * Per env e, for t = K-1 down to 0; `next` is the state of step t + 1, or the tail at t = K-1:
 *     the record's byte BG_ROW_TERMINATED is set:  steps = 0;  ante = the record's int16 BG_ROW_END_ANTE;  flags = its byte BG_ROW_END_FLAGS;  ret = r
 *     elsewhere:  steps = next.steps < 0 ? -1 : next.steps + 1;  ante = next.ante;  flags = next.flags;  ret = r + gamma * next.ret
 * r is the record's float64 reward, or rewards_dev[t][e] (dense float64 [K, N], as bg_gae_rows_ex; it needs returns_dev).  ret is float64, the product
 * and the sum each rounded, nothing fused.  The chain is serial in t per env, so every output is bit for bit that loop in numpy.
 * Outputs, dense [K, N], each nullable but at least one given: steps_to_end_dev int32, end_ante_dev int32, end_flags_dev uint8, returns_dev float64.
 * Each has a nullable tail input [N] -- the value BEHIND the last step: row 0 of the same call on the following chunk, so a long store is processed in
 * pieces from the back; a tail without its output is refused.  The defaults are -1, -1, 0 and 0.0: an episode that does not end inside the call and
 * has no tail is OPEN -- steps -1, ante -1, flags 0, ret the discounted sum so far.  end_ante is 0 in records written without the episode summary
 * (bg_set_episode_summary).  An output must not be the same pointer as an input or another output; gamma must not be NaN.
 *
 * bg_bc_loss (csrc/bg_bc.h, where every order of evaluation is fixed): the weighted cross-entropy of stored actions under the masked head above, its
 * accuracy and its gradient with respect to the logits, in one pass over the logits.  Row i reads its logits at i; with index_dev (int32 [m]) the
 * STORED arrays -- mask, actions, weights -- are read at row src = index[i] of store_rows rows, else at i.  The action is the int32 at actions_dev +
 * src * actions_stride_bytes (a multiple of 4, >= 4: 4 is a dense array; a record pitch reads BG_ROW_ACTION in place -- the demonstration of
 * observation record t is the action in record t + 1, so actions_dev = rows_dev + row_stride_bytes * N + BG_ROW_ACTION for a [K + 1, N] store); the
 * mask as in bg_ppo_loss; weights_dev float32 [store_rows], nullable (w = 1).  m_, d[j], e[j], S, A, logS, H are bg_head_row's: log_prob and entropy
 * are bit for bit bg_evaluate_actions'.  All arithmetic is float32, every operation rounded on its own; the sums across rows are float64.
 *     W  = the float64 sum of the weights of all rows whose index is in range and whose weight is finite and >= 0 (m without weights and index);
 *          Wf = float(W);  W == 0: loss 0 and an all-+0.0 gradient
 *     nll = 0 - log_prob;  hit = 1 where the first maximum among the valid logits is the action (bg_sample_actions' deterministic rule), else 0
 *     p = e[j] / S;  valid j with e[j] > 0:  dlogits[i, j] = (((ent_coef * p) * ((d[j] - logS) + H) - (1[j == a] - p)) * w) / Wf
 *     valid j with e[j] == 0: ((0 - 1) * w) / Wf if j == a, else +0.0;  invalid j: +0.0;  padding columns of a strided dlogits are not written
 *     nll_loss = sum(w nll) / W;  entropy_loss = -sum(w H) / W;  accuracy = sum(w hit) / W;  loss = nll_loss + ent_coef * entropy_loss
 *     (float64 from the float64 sums, each scalar rounded to float32 once)
 * An EXCLUDED row -- degenerate for the head, action outside [0, 60) or masked, log_prob not finite, weight not finite or negative, index outside
 * [0, store_rows) (nothing is read for it; log_prob = entropy = quiet NaN) -- adds nothing to any sum, has a +0.0 dlogits row and is counted; rows
 * excluded for another reason than their index or weight stay in W, as m stays PPO's divisor.  The sums take bg_ppo_loss' fixed orders (no floating-
 * point atomics): two calls give the same bits.  stats_dev, float32 [BG_BC_STATS]: loss, nll_loss, entropy_loss, accuracy, weight_sum, excluded rows,
 * m.  dlogits_dev has the dtype of the logits and its own row stride (>= 60); log_prob_dev, entropy_dev may be NULL.  workspace_dev: 16-byte aligned,
 * bg_bc_loss_workspace_bytes(m) bytes.  BG_E_ARG (text "bg_bc_loss: ..." in bg_last_error(NULL)) before anything is launched for: wrong alignment, a
 * stride < 60, an actions stride that is no multiple of 4, an output that is the same pointer as an input or another output, a non-finite ent_coef, a
 * workspace too small.  m == 0 writes zeros to stats_dev and launches nothing else.  Never synchronises unless timing is asked for.
 * Out of scope: label smoothing, an L2 term (the optimiser's weight decay), (the demonstration ring is bg_demo_append_rows; the expert policy is bg_expert_actions). */
int bg_episode_outcome_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N, double gamma,
                            const double* rewards_dev /*nullable*/,
                            const int32_t* tail_steps_dev /*nullable*/, const int32_t* tail_ante_dev /*nullable*/,
                            const uint8_t* tail_flags_dev /*nullable*/, const double* tail_return_dev /*nullable*/,
                            int32_t* steps_to_end_dev /*nullable*/, int32_t* end_ante_dev /*nullable*/,
                            uint8_t* end_flags_dev /*nullable*/, double* returns_dev /*nullable*/,
                            float* kernel_ms_out, void* stream);
#define BG_BC_STATS 7
uint64_t bg_bc_loss_workspace_bytes(int64_t m);
int bg_bc_loss(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems,
               const int8_t* mask_dev /*nullable*/, uint64_t mask_stride_bytes,
               const int32_t* actions_dev, uint64_t actions_stride_bytes,
               const float* weights_dev /*nullable*/,
               const int32_t* index_dev /*nullable*/, int64_t store_rows, int64_t m, float ent_coef,
               void* dlogits_dev, uint64_t dlogits_stride_elems,
               float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
               float* stats_dev /* float32[BG_BC_STATS = 7] */,
               void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);

/* DQN over packed records: the temporal-difference loss of SB3's `DQN.train`, its gradient with respect to the online Q values and its diagnostics, in
 * one pass over the minibatch; and epsilon-greedy exploration in the masked head above.  The arithmetic and the order of every operation are
 * csrc/bg_dqn.h.  Replaces: the DQN branch of the reference's main training script (`--algorithm {PPO, DQN, A2C}`, train_balatro_agent.py:344-362:
 * buffer_size 100 000, batch_size 32, exploration 1.0 -> 0.05, target_update_interval 1000, tau 1.0) between "two [m, 60] Q matrices" and "a gradient":
 * gather -> masked max -> where(done) -> multiply-add -> smooth_l1_loss -> mean, and their backward.
 *
 * A ring of records is the replay buffer: record nx = next_index[i] is the transition's NEXT record and holds the action (BG_ROW_ACTION), the reward
 * (BG_ROW_REWARD), BG_ROW_TERMINATED and BG_ROW_END_FLAGS of the step that produced it, and the action mask (BG_ROW_ACTION_MASK) of the next decision;
 * the observation record is not an argument (the caller computed q from it).  q_dev [m, 60]: the online network at the observation records;
 * q_next_dev [m, 60]: the target network at the next records; q_next_online_dev [m, 60], nullable: the online network at the next records (non-NULL
 * selects double DQN).  All three BG_HEAD_F32 or BG_HEAD_BF16 (q_dtype; widened exactly), each with its own row stride >= 60 under the alignment rules
 * of bg_ppo_loss.  rewards_dev float32 [store_rows], nullable: read at next_index[i] instead of the record's float64 reward (normalised rewards, as
 * bg_gae_rows_ex).  All arithmetic is float32, every operation rounded on its own (no fused multiply-add); the sums across rows are float64:
 *     a = record action;  r = float(record reward) or rewards[next_index[i]];  done = terminated != 0
 *     V' = the j whose next-record mask byte is non-zero (BG_DQN_MASK_NEXT), else all 60
 *     plain:   n = max over V' of q_next[j]
 *     double:  a' = the smallest j in V' with q_next_online[j] == max over V' of q_next_online;  n = q_next[a']
 *     y = done ? r : r + gamma * n          (a done row reads neither q_next matrix: a NaN there does not matter)
 *     d = q[a] - y
 *     Huber (SB3's smooth_l1, beta 1):  term = |d| < 1 ? (0.5 * d) * d : |d| - 0.5;  g = |d| < 1 ? d : copysign(1, d)
 *     BG_DQN_MSE:                        term = d * d;  g = 2 * d
 *     dq[i, a] = g / float(m);  every other column of the row +0.0;  padding columns of a strided dq are not written;  td[i] = d
 * An EXCLUDED row -- next_index outside [0, store_rows) (nothing is read for it); the action outside [0, 60) (the record carries the caller's value as
 * given); r or q[a] not finite; not done and V' empty, a Q value that enters a max NaN, or n not finite; BG_DQN_TIMEOUT_EXCLUDE set, done and
 * end_flags == BG_END_MAX_STEPS exactly -- has a dq row of +0.0 and td = quiet NaN, adds nothing to any sum, is counted, and the divisor stays m.
 * The last rule is the step-limit ending: SB3 bootstraps such a row from `terminal_observation`, a record that is not in the ring; without the flag it
 * is an ordinary done row.  Bootstrapping it from the terminal record is out of scope.
 * dq_dev: the dtype of q (bfloat16: the float32 value rounded to nearest even), its own stride.  td_dev float32 [m], nullable (for prioritised replay).
 * stats_dev float32 [BG_DQN_STATS], each from float64 sums over the included rows rounded to float32 once: loss = (sum term) / m, mean q[a], mean y,
 * mean |d| (each sum / m), max |d|, the share of done rows, the number of excluded rows, m.  The sums take a fixed order (64 rows per workgroup by a
 * tree, the workgroups' partials from workspace_dev in index order by slices and a tree in a one-workgroup kernel; no floating-point atomics): two calls
 * give the same bits.  workspace_dev: 16-byte aligned, bg_dqn_loss_workspace_bytes(m) bytes.
 * BG_E_ARG (text "bg_dqn_loss: ..." in bg_last_error(NULL)) before anything is launched for: wrong alignment, a stride < 60, a row stride below
 * BG_ROW_BYTES or no multiple of 16, an output that is the same pointer as an input or another output, gamma not finite or outside [0, 1],
 * store_rows >= 2**31, a workspace too small, unknown flags.  m == 0 writes zeros to stats_dev and launches nothing else.  Never synchronises unless
 * timing is asked for.  Out of scope: Polyak / hard target updates, the optimiser, gradient clipping, prioritised sampling, n-step returns.
 *
 * bg_sample_actions_eps: bg_sample_actions' arguments plus epsilon in [0, 1]; flags must be 0 and log_prob_dev / entropy_dev NULL.
 *     h = bg_policy_hash(seed, index0 + i, t) and u = float(h >> 8) * 2^-24 as bg_sample_actions;  explore = u < epsilon (exact float32 comparison)
 *     greedy rows take the BG_HEAD_DETERMINISTIC rule;  exploring rows take h2 = bg_policy_hash(seed + 0x632BE59BD9B4E019 mod 2^64, index0 + i, t) and,
 *     with k the number of valid actions, the ((uint64)h2 * k) >> 32 -th valid action in index order;  a degenerate row gives -1 in both branches.
 * DEVIATION from SB3: the decision is per env.  SB3 draws once for the whole batch, which at 65 536 envs would make every env explore together. */
#define BG_DQN_STATS 8
#define BG_DQN_MASK_NEXT 1u       /* flags: the max / argmax at the next record runs over its action mask */
#define BG_DQN_MSE 2u             /* flags: squared error instead of Huber */
#define BG_DQN_TIMEOUT_EXCLUDE 4u /* flags: leave out rows that only the step limit ended */
uint64_t bg_dqn_loss_workspace_bytes(int64_t m);
int bg_dqn_loss(const void* q_dev, uint64_t q_stride_elems, const void* q_next_dev, uint64_t q_next_stride_elems,
                const void* q_next_online_dev /*nullable*/, uint64_t q_next_online_stride_elems, int q_dtype,
                const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                const int32_t* next_index_dev, const float* rewards_dev /*nullable*/, int64_t m,
                float gamma, uint32_t flags,
                void* dq_dev, uint64_t dq_stride_elems, float* td_dev /*nullable*/,
                float* stats_dev /* float32[BG_DQN_STATS = 8] */,
                void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);
int bg_sample_actions_eps(const void* logits_dev, int logits_dtype, uint64_t logits_stride_elems,
                          const int8_t* mask_dev, uint64_t mask_stride_bytes, int64_t m, uint32_t flags,
                          uint64_t seed, uint64_t index0, uint64_t t, float epsilon,
                          int32_t* actions_dev, float* log_prob_dev /*must be NULL*/, float* entropy_dev /*must be NULL*/,
                          float* kernel_ms_out, void* stream);

/* The network's first layer straight from the stored records, on the matrix cores, forward and backward: the features of bg_encode_rows_ex are built in
 * LDS and multiplied with the weight in the same launch, so the [m, 628] feature matrix exists neither for the forward pass nor for the weight gradient.
 * The arithmetic and the tile shapes are csrc/bg_linear.h.
 * Replaces: `CombinedExtractor`'s concatenation plus the first `nn.Linear` of `mlp_extractor` under `PPO("MultiInputPolicy", ...)` over
 * `BalatroEnvFixed` -- 628 inputs into first layers of 512 units for policy and value (hpc_train.py:92-93, train_balatro_fixed.py:361-363) -- which
 * runs once per collected step and n_epochs = 10 times per rollout, and the autograd backward of that layer.  475 of the 628 columns are the keys
 * BalatroEnvFixed zero-fills (exactly 0.0 with frozen statistics too), so the reduction runs over the 153 produced columns; a first layer needs no
 * gradient with respect to its input, so the backward pass is dweight and dbias alone.
 *
 * bg_linear_rows:       out[i, n] = act( sum over k < 153 of x[i, k] * w[n, k]  +  b[n] )
 * x[i, :] = the first 153 columns of the row bg_encode_rows_ex writes with out_dtype BG_ENC_BF16 for the same rows_dev, row_stride_bytes, store_rows,
 * index_dev, m, mean_dev / var_dev, epsilon, clip_obs -- bit for bit: the float32 value, then round to nearest even to bfloat16.  An index outside
 * [0, store_rows) reads nothing and gives x = 0, so out = act(b).  layout BG_ENC_PRODUCED or BG_ENC_FIXED: identical results (columns 153..627 are
 * zero and are never read from the weight); BG_ENC_EXTRACTOR is a BG_E_ARG (its 416 one-hot columns want an embedding gather).
 * weight_dev: bfloat16 in torch's `nn.Linear.weight` orientation, [H, weight_stride_elems >= 153] (at most 2**24); a [H, 628] weight is passed in place and only its
 * first 153 columns are read; 2-byte alignment is all that is required.  bias_dev: float32 [H] or NULL.  activation: BG_LIN_NONE, or BG_LIN_RELU =
 * max(v, +0.0) (a NaN stays a NaN).  out_dtype BG_ENC_F32 or BG_ENC_BF16, out_stride_elems >= H; columns at or beyond H and rows at or beyond m are
 * not touched.  H: a multiple of 32 in [32, 4096] (policy and value first layers run as one call on the concatenated weight).
 * Products are bfloat16 x bfloat16 (exact in float32), accumulated in float32 by __builtin_amdgcn_mfma_f32_32x32x16_bf16 over the reduction padded to
 * 160 with zeros; the bias is added in float32 behind the sum, then the activation, then ONE rounding to the output dtype.  The order inside the product
 * is the instruction's own and a fixed function of (m, H): two calls give the same bits.
 *
 * bg_linear_rows_grad:  dweight[n, k] = sum over i of dp[i, n] * x[i, k]  (k < 153);    dbias[n] = sum over i of dp[i, n]
 * x is the forward's, rebuilt from the records with the same arguments.  dp[i, n] = bfloat16(dout[i, n]) (round to nearest even; dout_dtype BG_ENC_F32
 * or BG_ENC_BF16, dout_stride_elems >= H); with BG_LIN_RELU, dp[i, n] is that where out[i, n] > 0 and +0.0 elsewhere: out_dev / out_dtype /
 * out_stride_elems are the forward's output, required exactly when the flag is set (NULL otherwise).  dweight_dev: float32 [H, dweight_stride_elems >=
 * 153], columns at or beyond 153 untouched (their exact gradient is zero: the caller's business); dbias_dev: float32 [H] or NULL.  There is no gradient
 * with respect to the records.  The sum over i has no floating-point atomics: the rows are cut into groups of consecutive 128-row blocks, a workgroup
 * keeps float32 matrix-core accumulators over the rows of its group (its dbias sum: float32 in row order per lane), the groups' partials ([161, H]
 * float32 each) go to workspace_dev and a second launch adds them in index order in float64, rounding once.  bg_linear_rows_workspace_bytes(m, H) =
 * groups * 161 * H * 4 bytes, groups = ceil(B / ceil(B / max(1, 256 / ceil(H / 256)))) with B = ceil(m / 128): at most 256 partials, 42 MB at H >= 256;
 * a group holds 128 * ceil(B / groups) rows at most.  workspace_dev: 16-byte aligned.  Two calls give the same bits.
 *
 * Both calls run on the current device, need no handle, return BG_E_ARG (text "bg_linear_rows: ..." / "bg_linear_rows_grad: ..." in
 * bg_last_error(NULL)) before anything is launched, treat m == 0 as a no-op and never synchronise unless timing is asked for; kernel_ms_out as in
 * bg_classify_batch_ex.  All record addressing is 64-bit.
 * Out of scope: the extractor layout, tanh and other activations, a gradient with respect to the records, statistics updates, fp8 / MX formats,
 * deeper layers and the optimiser. */
#define BG_LIN_NONE 0
#define BG_LIN_RELU 1
int bg_linear_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                   const int32_t* index_dev /*nullable*/, int64_t m, int layout,
                   const double* mean_dev /*nullable*/, const double* var_dev /*nullable*/, double epsilon, double clip_obs,
                   const void* weight_dev, uint64_t weight_stride_elems, const float* bias_dev /*nullable*/, int H, int activation,
                   int out_dtype, void* out_dev, uint64_t out_stride_elems, float* kernel_ms_out, void* stream);
uint64_t bg_linear_rows_workspace_bytes(int64_t m, int H);
int bg_linear_rows_grad(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                        const int32_t* index_dev /*nullable*/, int64_t m, int layout,
                        const double* mean_dev /*nullable*/, const double* var_dev /*nullable*/, double epsilon, double clip_obs,
                        const void* dout_dev, int dout_dtype, uint64_t dout_stride_elems,
                        const void* out_dev /*nullable*/, int out_dtype, uint64_t out_stride_elems, int H, int activation,
                        float* dweight_dev, uint64_t dweight_stride_elems, float* dbias_dev /*nullable*/,
                        void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);

/* The first layer behind BalatroFeaturesExtractor's input, straight from the stored records, forward and backward -- the counterpart of bg_linear_rows
 * for the one layout it refuses.  The arithmetic and the tile shapes are csrc/bg_extractor.h.
 * Replaces: the tensors `BalatroFeaturesExtractor.forward` builds (train_balatro_agent.py:84-119: the hand one-hot :86-93, `joker_ids.float()` :98,
 * `game_features` :102-113) plus the first `nn.Linear` of `hand_net`, `joker_net` and `game_state_net`, which PPO, DQN and A2C of that script
 * (:326-377) all run, and the autograd backward of those layers.  The three layers are ONE call on a block-structured [h + j + s, 447] weight.
 *
 * bg_extractor_rows:       out[i, n] = act( sum over k < 447 of x[i, k] * w[n, k]  +  b[n] )
 * x[i, :] = the row bg_encode_rows_ex writes with layout BG_ENC_EXTRACTOR and out_dtype BG_ENC_BF16 for the same rows_dev, row_stride_bytes,
 * store_rows, index_dev, m -- bit for bit, and never written: column 52 slot + card is 1.0 where hand byte `slot` equals `card` (card in 0..51; the
 * bytes -1, 52..127 and negative values match no column; the same card in two slots sets two columns), the other 31 columns are the float32 values
 * rounded to nearest even to bfloat16.  An index outside [0, store_rows) reads nothing and gives x = +0.0, so out = act(b).  There are no VecNormalize
 * statistics: every call refuses them for this layout, and this one does not take them.
 * weight_dev: bfloat16 in torch's `nn.Linear.weight` orientation, [H, weight_stride_elems >= 447] (at most 2**24); 2-byte alignment is all that is
 * required (a 16-byte aligned matrix with a pitch that is a multiple of 8, e.g. 448, is staged fastest).  bias_dev: float32 [H] or NULL.  activation:
 * BG_LIN_NONE or BG_LIN_RELU, as bg_linear_rows.  out_dtype BG_ENC_F32 or BG_ENC_BF16, out_stride_elems >= H; columns at or beyond H and rows at or
 * beyond m are not touched.  H: a multiple of 32 in [32, 4096].
 * Products are bfloat16 x bfloat16 (exact in float32), accumulated in float32 by __builtin_amdgcn_mfma_f32_32x32x16_bf16 over the reduction padded to
 * 448 with a zero; the bias is added in float32 behind the sum, then the activation, then ONE rounding to the output dtype: a bfloat16 output is the
 * round-to-nearest-even of the float32 output of the same arithmetic.  Two calls give the same bits.
 *
 * bg_extractor_rows_grad:  dweight[n, k] = sum over i of dp[i, n] * x[i, k]  (k < 447);    dbias[n] = sum over i of dp[i, n]
 * dp, dout_*, out_* as bg_linear_rows_grad: dp = bfloat16(dout), +0.0 where BG_LIN_RELU's forward output is not > 0 (out_dev required exactly then).
 * dweight_dev: float32 [H, dweight_stride_elems >= 447], columns at or beyond 447 untouched; dbias_dev: float32 [H] or NULL.  The rows are cut into
 * groups of consecutive 128-row blocks, the units into spans of 256 and k into 3 spans of 160, 160 and 128 columns; a workgroup keeps float32
 * matrix-core accumulators over the rows of its group, the groups' partials ([449, H] float32 each: dweight^T and the dbias row) go to workspace_dev
 * and a second launch adds them in index order in float64, rounding once.  There are no atomics: two calls give the same bits.
 * bg_extractor_rows_workspace_bytes(m, H) = groups * 449 * H * 4 bytes, groups = ceil(B / ceil(B / max(1, 256 / (3 * ceil(H / 256))))) with
 * B = ceil(m / 128): at most 256 workgroups, 39 MB at the most; a group holds 128 * ceil(B / groups) rows at most.  workspace_dev: 16-byte aligned.
 *
 * Both calls run on the current device, need no handle, return BG_E_ARG (text "bg_extractor_rows: ..." / "bg_extractor_rows_grad: ..." in
 * bg_last_error(NULL)) before anything is launched, treat m == 0 as a no-op and never synchronise unless timing is asked for; kernel_ms_out as in
 * bg_classify_batch_ex.  All record addressing is 64-bit.
 * Out of scope: the second layers of the three sub-networks and `combined_net`, skipping the structurally zero blocks of a block-structured weight,
 * tanh, a gradient with respect to the records, and the optimiser. */
int bg_extractor_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                      const int32_t* index_dev /*nullable*/, int64_t m,
                      const void* weight_dev, uint64_t weight_stride_elems, const float* bias_dev /*nullable*/,
                      int H, int activation, int out_dtype, void* out_dev, uint64_t out_stride_elems,
                      float* kernel_ms_out, void* stream);
uint64_t bg_extractor_rows_workspace_bytes(int64_t m, int H);
int bg_extractor_rows_grad(const uint8_t* rows_dev, uint64_t row_stride_bytes, int64_t store_rows,
                           const int32_t* index_dev /*nullable*/, int64_t m,
                           const void* dout_dev, int dout_dtype, uint64_t dout_stride_elems,
                           const void* out_dev /*nullable*/, int out_dtype, uint64_t out_stride_elems,
                           int H, int activation,
                           float* dweight_dev, uint64_t dweight_stride_elems, float* dbias_dev /*nullable*/,
                           void* workspace_dev, uint64_t workspace_bytes,
                           float* kernel_ms_out, void* stream);

/* The policy's last layer fused with the masked head and with PPO's loss: bg_sample_actions, bg_evaluate_actions and bg_ppo_loss with
 * (h, weight, bias) in place of the logits.  The arithmetic, the kernels' shape and the serial twin are csrc/bg_actor.h.
 * Replaces: SB3's `action_net` = nn.Linear(latent, 60) (latent 256 or 512 in every training script of the reference), the [m, 60] logits matrix it
 * writes for the head to read back, and on the training side the gradient's three more trips: dlogits written by bg_ppo_loss and read twice by the
 * autograd backward of the layer (dlogits^T @ h and dlogits @ W).  Here a workgroup takes 64 rows of h, the matrix cores
 * (__builtin_amdgcn_mfma_f32_32x32x16_bf16) put their logits tile into LDS, the row functions of the head / the loss run on it unchanged, and for
 * training two more products consume the gradient tile before it leaves the CU.
 *
 * h_dev: bfloat16 [m, Hin], row i at element i * h_stride_elems; the pointer 16-byte aligned, the stride a multiple of 8, >= Hin.  Hin: a multiple of 32
 * in [32, 1024]; LDS does not grow with it.  weight_dev: [60, Hin] (nn.Linear.weight's orientation) BG_ENC_F32 or BG_ENC_BF16, row j at element
 * j * weight_stride_elems (>= Hin), aligned to its element; a float32 weight is rounded to bfloat16 on load (nearest even, NaN -> 0x7fc0): w_b.
 * bias_dev: float32 [60] or NULL.  mask, seed, index0, t, flags: exactly bg_sample_actions' / bg_evaluate_actions'; mask, actions, old_log_prob,
 * advantages, values, returns, index_dev, store_rows, clip_range, ent_coef, vf_coef, flags, dvalues, log_prob, entropy, stats: exactly bg_ppo_loss'.
 *     logit[i][j] = float32(sum over k of h[i][k] * w_b[j][k]) + bias[j]
 * Every product is exact; the sum is the float32 accumulation of the instruction over k in ascending blocks of 16, the 60 units padded to 64 with zero
 * weights (padding units never reach the head); the bias is one float32 addition behind the sum (NULL: no addition).  The logits are bounded against
 * float64 (tests/actor_ref.py), not promised bit for bit against another accumulation order.  logits_out_dev (float32 [m, stride >= 60], nullable)
 * returns them, and GIVEN them everything behind is exact: actions, log_prob and entropy are bit for bit what bg_sample_actions / bg_evaluate_actions
 * return for logits_out with the same mask, seed, index0 and t, whether logits_out_dev is given or not; bg_actor_ppo_loss' stats, log_prob, entropy,
 * dvalues and dlogits_out_dev (float32 [m, stride >= 60], nullable) are bit for bit bg_ppo_loss' on logits_out -- the launch sequence is that call's,
 * its advantage-statistics kernels and its finishing kernel are reused, and the fused rows kernel writes the same six float64 sums per 64 rows.
 *
 * bg_actor_ppo_loss writes, in place of dlogits, the gradients of the layer.  dp[i][j] = bfloat16(dlogits[i][j]) (nearest even; an excluded row: +0.0).
 *     dh[i][k]      = float32(sum over j of dp[i][j] * w_b[j][k])          dh_dev BG_ENC_F32 or BG_ENC_BF16 [m, dh_stride_elems >= Hin]; a bfloat16 dh is
 *                                                                            the nearest-even rounding of that float32 value; an excluded row is +0.0
 *     dweight[j][k] = sum over i of dp[i][j] * h[i][k]                     float32 [60, Hin], dense
 *     dbias[j]      = sum over i of dp[i][j]                               float32 [60]
 * dweight and dbias are accumulated in float32 inside a row group -- bg_actor_ppo_loss_rows_per_group(m, Hin) consecutive rows: blocks of 64 rows,
 * ceil(B / cap) blocks per group with B = ceil(m / 64) and cap = 256 / ceil(Hin / 256) -- and the groups' partials (workspace) are summed in float64 in
 * index order and rounded once: bg_linear_rows_grad's scheme.  No floating-point atomics: two calls give the same bits.
 * NON-FINITE INPUTS: a NaN or an infinity in h, weight or bias is carried into the logits it touches and the head's rules decide from there -- at a
 * valid unit a NaN or +inf makes the row degenerate (action -1, NaN) or excluded from the loss, at a masked unit it is ignored.  The gradient products are
 * plain IEEE arithmetic: +0.0 times a non-finite operand is NaN, so dh / dweight / dbias are finite only where the operands they multiply are.
 * workspace_dev: 16-byte aligned, bg_actor_ppo_loss_workspace_bytes(m, Hin) bytes = bg_ppo_loss_workspace_bytes(m) rounded up to 16, plus
 * groups * (60 * Hin + 64) * 4.  All three calls run on the current device, need no handle and never synchronise unless timing is asked for.
 * BG_E_ARG (text "bg_actor_sample: ..." / "bg_actor_evaluate: ..." / "bg_actor_ppo_loss: ..." in bg_last_error(NULL)) before anything is launched for:
 * everything bg_sample_actions / bg_evaluate_actions / bg_ppo_loss refuse; Hin out of range; h_dev misaligned or its stride not a multiple of 8; a stride
 * below its width; an unknown dtype; an output that is the same pointer as an input or another output; a workspace too small.  m == 0: the head calls
 * are no-ops; bg_actor_ppo_loss zeroes stats_dev, dweight_dev and dbias_dev and launches nothing else.
 * Out of scope: the value head, DQN's and behaviour cloning's last layers, epsilon-greedy, temperature, Hin not a multiple of 32. */
int bg_actor_sample(const void* h_dev, uint64_t h_stride_elems, int Hin,
                    const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems, const float* bias_dev /*nullable*/,
                    const int8_t* mask_dev /*nullable*/, uint64_t mask_stride_bytes, int64_t m, uint32_t flags,
                    uint64_t seed, uint64_t index0, uint64_t t,
                    int32_t* actions_dev, float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
                    float* logits_out_dev /*nullable*/, uint64_t logits_out_stride_elems,
                    float* kernel_ms_out, void* stream);
int bg_actor_evaluate(const void* h_dev, uint64_t h_stride_elems, int Hin,
                      const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems, const float* bias_dev /*nullable*/,
                      const int8_t* mask_dev /*nullable*/, uint64_t mask_stride_bytes, int64_t m,
                      const int32_t* actions_dev, float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
                      float* logits_out_dev /*nullable*/, uint64_t logits_out_stride_elems,
                      float* kernel_ms_out, void* stream);
uint64_t bg_actor_ppo_loss_workspace_bytes(int64_t m, int Hin);
int64_t bg_actor_ppo_loss_rows_per_group(int64_t m, int Hin);
int bg_actor_ppo_loss(const void* h_dev, uint64_t h_stride_elems, int Hin,
                      const void* weight_dev, int weight_dtype, uint64_t weight_stride_elems, const float* bias_dev /*nullable*/,
                      const int8_t* mask_dev /*nullable*/, uint64_t mask_stride_bytes,
                      const int32_t* actions_dev, const float* old_log_prob_dev, const float* advantages_dev,
                      const float* values_dev /*nullable*/, const float* returns_dev /*nullable*/,
                      const int32_t* index_dev /*nullable*/, int64_t store_rows, int64_t m,
                      float clip_range, float ent_coef, float vf_coef, uint32_t flags,
                      void* dh_dev, int dh_dtype, uint64_t dh_stride_elems, float* dweight_dev, float* dbias_dev,
                      float* dvalues_dev /*nullable*/, float* log_prob_dev /*nullable*/, float* entropy_dev /*nullable*/,
                      float* stats_dev /* float32[BG_PPO_STATS = 10] */,
                      float* logits_out_dev /*nullable*/, uint64_t logits_out_stride_elems,
                      float* dlogits_out_dev /*nullable*/, uint64_t dlogits_out_stride_elems,
                      void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);

/* ---- bg_optim_step: gradient clipping, Adam / RMSpropTFLike, the L2 term, the bfloat16 weight copies and DQN's target update, for ALL parameter
 * tensors in three launches (csrc/bg_optim.h has the contract, the kernels and the serial twin; tests/optim_ref.py restates it in numpy).
 * Replaces: `clip_grad_norm_(params, 0.5); optimizer.step(); optimizer.zero_grad()` of every training script of the reference (max_grad_norm 0.5;
 * Adam with SB3's eps 1e-5 for PPO and DQN; SB3's RMSpropTFLike for `--algorithm A2C`), the per-call float32 -> bfloat16 weight casts of the first
 * layers and the actor, and SB3's polyak_update of DQN's target network (tau 1.0 every 1000 steps).
 *
 * table_dev: 16-byte aligned; ntensors (<= 1024) entries of 64 bytes --
 *     float* param, grad, state1, state2;  uint16_t* shadow (nullable);  float* target (nullable);  uint64_t numel;  uint32_t cols, pitch;
 * every float32 array contiguous with numel elements (4-byte aligned; four 16-byte aligned pointers take the 16-byte path), shadow bfloat16 with
 * element i at (i / cols) * pitch + i % cols, pitch >= cols >= 1 -- followed by uint32 prefix[ntensors + 1]: prefix[t] = the chunks of the tensors
 * before t, a tensor having ceil(numel / 1024) chunks (numel >= 1).  chunks = prefix[ntensors].  The library trusts the table: it is device memory.
 * carry_dev: 32 bytes owned by the caller's optimiser and carried from call to call: int64 step, float64 b1pow, float64 b2pow, 8 bytes unused; start it
 * at (0, 1.0, 1.0).  workspace_dev: 16-byte aligned, bg_optim_workspace_size(chunks) bytes = 32 + 16 * chunks.  stats_dev: BG_OPTIM_STATS_BYTES bytes:
 * float32 grad_norm, float32 clip_coef, int32 skipped, int32 0, int64 nonfinite, int64 step.
 *     norm  = float32(sqrt(sum of (double)g * (double)g))   in THE REDUCTION ORDER of bg_ppo.h over chunks of 1 024 elements: the same bits on every run
 *     c     = min(1, max_norm / (norm + 1e-6f)), or 1 with max_norm <= 0
 *     a non-finite norm SKIPS the step: nothing but the gradients (BG_OPTIM_ZERO_GRAD) is written and the carried state is not advanced
 *     g = g * c;  g = g + p * weight_decay (when non-zero)
 *     BG_OPTIM_ADAM:        m = m + (g - m) * (1 - beta1);  v = v * beta2 + ((1 - beta2) * g) * g;  p = p + (m / (sqrt(v) / s2 + eps)) * (-a)
 *                           a = float32(lr / (1 - beta1 ** step)), s2 = float32(sqrt(1 - beta2 ** step)), the powers carried as iterated float64 products
 *     BG_OPTIM_RMSPROP_TF:  sq = sq * alpha + ((1 - alpha) * g) * g;  p = p + (g / sqrt(sq + eps)) * (-lr)     (state1 = sq starts at ones, state2
 *                           unused and may be NULL; alpha travels in beta1)
 *     shadow = bfloat16(p) to nearest even;  with tau > 0: target = target * (1 - tau) + p * tau (tau == 1: a copy);  BG_OPTIM_ZERO_GRAD: grad = 0
 * every operation a float32 one rounded on its own.  BG_OPTIM_SHADOW_ONLY: one launch that writes the shadows from the current parameters and nothing
 * else; carry_dev, workspace_dev and stats_dev may be NULL then.  The call never synchronises unless timing is asked for: the step count and the bias
 * corrections live on the device.
 * BG_E_ARG (text "bg_optim_step: ..." in bg_last_error(NULL)) before anything is launched for: ntensors outside [0, 1024]; chunks not in
 * [ntensors, 2**31) or zero for a non-empty table; an unknown algo or flag; lr, eps or weight_decay negative or not finite; a beta outside [0, 1); tau
 * outside [0, 1]; a NULL or misaligned block; two blocks at one address.  An empty table returns 0 and launches nothing.
 * Out of scope: AdamW, amsgrad, momentum or centred RMSprop, parameter groups, sparse or non-float32 parameters, lr as a device scalar, multi-GPU
 * gradient reduction. */
#define BG_OPTIM_ADAM 0
#define BG_OPTIM_RMSPROP_TF 1
#define BG_OPTIM_ZERO_GRAD 1u
#define BG_OPTIM_SHADOW_ONLY 2u
#define BG_OPTIM_MAX_TENSORS 1024
#define BG_OPTIM_CHUNK 1024
#define BG_OPTIM_STATS_BYTES 32
uint64_t bg_optim_workspace_size(int64_t chunks);
int bg_optim_step(const void* table_dev, int ntensors, int64_t chunks, int algo, double lr, double beta1 /* RMSprop: alpha */, double beta2, double eps,
                  double weight_decay, double max_norm, double tau, uint32_t flags, void* carry_dev, void* workspace_dev, void* stats_dev,
                  float* kernel_ms_out, void* stream);

/* ---- bg_demo_append_rows / bg_demo_sample: the kept demonstration steps of a finished store, compacted into a ring of self-contained records on the
 * device (csrc/bg_demo.h has the contract, the kernels and the serial twin; tests/demo_ref.py restates it in numpy).
 * Replaces: `self.expert_trajectories` of the reference's `BehavioralCloning` (train_balatro_agent.py:220-262) -- a dense data set that holds only the
 * steps of the kept episodes and grows call by call -- and the torch composite that would build it (`nonzero()`, which synchronises the host on the
 * count, two gathers of records through int64 indices, the patch copies and a ring write with wrap).
 *
 * rows_dev: the [K + 1, N] store of records (row_stride_bytes a multiple of 16, >= BG_ROW_BYTES).  Candidate row i = t * N + e, 0 <= t < K, pairs the
 * observation record store[t][e] with the next record store[t + 1][e].  weights_dev float32 [K * N]: row i is KEPT iff its weight is finite and > 0.
 * All of the call is integer work and is held bit for bit:
 *     kept = the kept rows of the call;  T0 = cursor[0] before it;  the rank r of a kept row = the number of kept rows with a smaller i
 *     the kept row of rank r goes to slot (T0 + r) mod capacity
 *     kept > capacity: the rows of rank r < kept - capacity are written nowhere -- the last `capacity` kept rows survive, no two meet in a slot
 *     afterwards cursor[0] = T0 + kept, cursor[1] = kept;  the ring holds min(cursor[0], capacity) records
 *     the record written = bytes 0..351 of the observation record with three fields of the step that followed:
 *         bytes 136..143 (BG_ROW_REWARD)  returns_dev[i] (float64 [K * N], nullable), else the next record's reward
 *         bytes 172..175 (BG_ROW_ACTION)  the next record's
 *         bytes 342..351 (BG_ROW_TERMINATED, BG_ROW_END_FLAGS, BG_ROW_END_ANTE, BG_ROW_END_ROUND, BG_ROW_END_CHIPS)  the next record's
 *     bytes 340..341 (boss_blind_active, boss_blind_type) are observation and stay;  bytes 352 and above of a ring slot are never written
 *     demo_weight_dev[slot] = weights_dev[i];  demo_source_dev[slot] = i (int32 [capacity], nullable)
 * A demo record is self-contained: the ring goes to bg_encode_rows_ex / bg_linear_rows / bg_extractor_rows as rows_dev, and to bg_bc_loss as mask_dev
 * (demo_dev + BG_ROW_ACTION_MASK, the ring's stride) and actions_dev (demo_dev + BG_ROW_ACTION, the ring's stride), with demo_weight_dev as weights.
 * cursor_dev: int64[2] on the device, carried by the caller from call to call (start it at zeros; cursor[0] >= 0); it never leaves the device.
 * workspace_dev: 16-byte aligned, bg_demo_workspace_bytes(K * N) bytes = 16 + 4 per 1 024 candidate rows, rounded up to 16.
 * Three launches (count per chunk, one scan, scatter per chunk), no atomics: two calls on the same inputs give the same bytes.  Never synchronises
 * unless timing is asked for.  N == 0 is a no-op.  BG_E_ARG (text "bg_demo_append_rows: ..." in bg_last_error(NULL)) before anything is launched
 * for: K < 1 with N > 0; K * N >= 2**31; capacity outside [1, 2**31); a stride below BG_ROW_BYTES or no multiple of 16; a record pointer that is not
 * 16-byte aligned; the ring overlapping the store; an output that is the same pointer as an input or another output; a workspace too small; a NULL
 * required pointer.
 *
 * bg_demo_sample: m uniform draws over the ring's filled slots, on the device.  filled = min(cursor[0], capacity);
 *     index[i] = (int32)(((uint64)h * filled) >> 32),  h = the counter hash of bg_sample_actions over (seed, index0 + i, t)
 * so a draw depends on (seed, index0 + i, t) alone, whatever m.  filled == 0 gives -1 on every row: the index bg_bc_loss excludes and
 * bg_encode_rows_ex zeroes.  The multiply-high draw is biased by at most filled / 2**32 per slot.  The slots of a full ring are all equally old as far
 * as a learner cares: the draw is over slots, not over age.
 * Out of scope: prioritised or age-aware sampling, deduplication of identical records, a ring shared between GPUs.  (The expert policy that fills the ring is bg_expert_actions.) */
uint64_t bg_demo_workspace_bytes(int64_t store_rows);
int bg_demo_append_rows(const uint8_t* rows_dev, uint64_t row_stride_bytes, int K, int64_t N,
                        const float* weights_dev, const double* returns_dev /*nullable*/,
                        uint8_t* demo_dev, uint64_t demo_stride_bytes, int64_t capacity,
                        float* demo_weight_dev, int32_t* demo_source_dev /*nullable*/,
                        int64_t* cursor_dev /* int64[2] */,
                        void* workspace_dev, uint64_t workspace_bytes, float* kernel_ms_out, void* stream);
int bg_demo_sample(const int64_t* cursor_dev, int64_t capacity, uint64_t seed, uint64_t index0, uint64_t t,
                   int32_t* index_dev, int64_t m, float* kernel_ms_out, void* stream);

/* ---- bg_expert_actions: a scripted expert policy over packed records, one action per record (csrc/bg_expert.h has the rule, the kernel and the
 * serial twin; tests/expert_ref.py restates the rule in numpy).
 * Replaces: the reference's expert_agent.py (`BalatroExpertAgent`), which calls three methods it never defines and whose evaluate_hand is
 * `len(cards) * 10  # Placeholder`.  Its intent is kept: in play enumerate every combination of up to five hand cards, value each, select the best set
 * card by card, then PLAY_HAND; in the shop buy a joker if one can be bought, otherwise leave.  The value is ScoringEngine.score_hand's formula
 * (scoring_engine.py:103-122) over bg_classify / bg_hand_base / bg_card_chips: (base chips at the hand's level + the cards' chips) * base mult.
 *
 * Stateless, no handle: record i is rows_dev + i * row_stride_bytes (index_dev NULL, m <= store_rows) or rows_dev + index_dev[i] * row_stride_bytes;
 * an index outside [0, store_rows) gives action -1 and detail 0.  actions_dev int32 [m]; detail_dev int32 [m], nullable:
 *     bits 0-7    T, the 8-bit slot mask the expert is selecting towards (the cards to play, or to discard)
 *     bits 8-11   the hand type of the best subset P
 *     bit 12      discard mode (T is a discard);  bit 13  FELLBACK: the intended action was masked (or the phase unknown) and the fallback order
 *                 45, 46, 47, 31, 55, 0, 1..59 gave the action -- -1 when the whole mask is zero
 *     bits 16-31  min(value(P), 65535)
 * and 0 outside the play phase but for FELLBACK.  By phase: blind select takes the first valid of 45, 46, 47 (never a skip); the shop buys the
 * cheapest valid joker slot (20 + i with shop_items[i] == 3, ties to the smaller i), else leaves with 31 (never a reroll); a pack is skipped with 55;
 * play is the subset search, PLAY_HAND when a discard is not worth it (no discards left, the last hand, value * hands_left >= the chips still
 * needed, or nothing else in the hand), else a DISCARD of the five cheapest cards outside P; stale selections are deselected first.  Between two
 * PLAY_HAND / DISCARD actions of an env lie at most 13 card toggles.  The action is the `actions` of bg_step_rows (collection) and the
 * `actions_dev` of bg_bc_loss (relabelling a finished store of the learner's own states).
 * One launch, no atomics, one store per output per record; the records are not written; two calls give the same bytes.  m == 0 is a no-op.
 * BG_E_ARG (text "bg_expert_actions: ..." in bg_last_error(NULL)) before anything is launched for: a stride below BG_ROW_BYTES or no multiple of 16;
 * a record, index or output pointer that is misaligned (16, 4, 4 bytes); m < 0 or m >= 2**31; m > store_rows without an index; store_rows >= 2**31
 * with one; an output that overlaps the records or is the same pointer as the index or the other output.
 * bg_expert_actions_ex: the same with the lane mapping chosen (lanes_per_record 1, 8 or 64 share one record's subsets; 0 = the library's choice)
 * and the kernel time by events on the stream (kernel_ms_out, nullable; asking for it synchronises).
 * Out of scope: consumables, packs, vouchers, rerolls, selling, joker-aware valuation, any search beyond one hand. */
int bg_expert_actions(const void* rows_dev, int64_t row_stride_bytes, int64_t m, const int32_t* index_dev, int64_t store_rows,
                      int32_t* actions_dev, int32_t* detail_dev /*nullable*/, void* stream);
int bg_expert_actions_ex(const void* rows_dev, int64_t row_stride_bytes, int64_t m, const int32_t* index_dev, int64_t store_rows,
                         int32_t* actions_dev, int32_t* detail_dev /*nullable*/, int lanes_per_record, float* kernel_ms_out, void* stream);

/* ---- bg_policy_forward: everything between the network's first layer and the env in ONE launch, for collection and evaluation (csrc/bg_policy.h
 * has the kernel and the serial twin; tests/policy_ref.py the float64 statement and the bounds).
 * Replaces: the hidden layers the reference's policies run in torch behind their first layer -- the extractor's second layers and combined_net
 * (train_balatro_agent.py:54-82), SB3's mlp_extractor (net_arch pi / vf, train_balatro_agent.py:338-342), action_net, the masked draw and value_net --
 * about twenty launches that each write an [m, <= 512] activation.  Here no hidden activation and no logits matrix is written.
 *
 * net: a BgPolicyNet in HOST memory, checked on every call and carried to the kernel as a launch argument (nothing is uploaded; a table outside the
 * envelope never reaches the kernel).  layer[] holds, in this order: n_trunk trunk layers, n_pi and n_vf branch layers (each section 0..4 layers; both
 * branches read the trunk's output, or h where the trunk is empty), the action layer [60, latent_pi], and with has_value the value layer
 * [1, latent_vf].  THE ENVELOPE: every width, in0 included, a multiple of 32 in [32, 512]; a layer's in_features is the width of what it reads; every
 * weight bfloat16 [out_features, in_features] in nn.Linear's orientation, 16-byte aligned, weight_stride_elems a multiple of 8 and >= in_features;
 * every bias float32 [out_features], required; activation BG_POLICY_ACT_* on hidden layers, NONE on the two last; vf layers need the value layer.
 * h_dev: bfloat16 [m, in0], 16-byte aligned, h_stride_elems a multiple of 8 and >= in0 (what bg_extractor_rows / bg_linear_rows write, or a column
 * slice of it).  The mask: as bg_sample_actions (records at stride 384 or int8 [m, 60]; NULL: every action valid).
 *     one layer   y[i][j] = act(float32(sum_k x[i][k] * w[j][k]) + b[j]), rounded to nearest-even bfloat16 for the next layer: the products are exact,
 *                 the sum is the float32 accumulation of __builtin_amdgcn_mfma_f32_32x32x16_bf16 over k in ascending 16-blocks, the bias ONE
 *                 float32 addition.  relu keeps a NaN.  tanh(y) = sign(y) * (1 - 2 / (expf(2 |y|) + 1)), every operation rounded to float32.
 *                 Bounded by tests/policy_ref.py, not promised bit for bit against another order of accumulation.
 *     last layers the 60 logits and the value stay float32.
 *     head        GIVEN these logits (logits_out_dev returns them) actions, log_prob and entropy are bit for bit bg_sample_actions' (flags 0 or
 *                 BG_HEAD_DETERMINISTIC, with seed, index0, t) / bg_evaluate_actions' (flags BG_POLICY_EVALUATE: actions_dev is read).
 *     outputs     actions_dev int32 [m]; log_prob_dev, entropy_dev, values_dev float32 [m], each nullable (values_dev needs has_value).
 *     test outputs  taps_dev bfloat16 [m, bg_policy_tap_cols(net)] at taps_stride_elems: every hidden layer's output in table order; logits_out_dev
 *                 float32 [m, 60] at logits_out_stride_elems.  Asking for them changes no other output bit.
 * A row's outputs depend on its own inputs and (seed, index0 + i, t) only: not on m, not on the launch shape; two calls give the same bits.
 * LDS does not grow with the net: three activation images of 32 rows x 520 bfloat16.  One launch on `stream` of the current device, no workspace, no
 * handle; m == 0 is a no-op; kernel_ms_out as in bg_classify_batch_ex.  bg_policy_check(net): 0, or BG_E_ARG with the text in bg_last_error(NULL).
 * BG_E_ARG (text "bg_policy_forward: ..." in bg_last_error(NULL)) before anything is launched for: a net outside the envelope; flags other than the
 * three; a misaligned pointer or pitch; values_dev without has_value; an output that is the same pointer as an input or as another output.
 * Out of scope: a backward pass (training keeps autograd for the hidden layers), DQN's epsilon draw, a temperature, the first layer inside the same
 * launch, a network policy inside the rollout engine. */
#define BG_POLICY_ACT_NONE 0
#define BG_POLICY_ACT_RELU 1
#define BG_POLICY_ACT_TANH 2
#define BG_POLICY_EVALUATE 2u /* flags, beside BG_HEAD_DETERMINISTIC */
#define BG_POLICY_MAX_SECTION 4
#define BG_POLICY_MAX_LAYERS 14
#define BG_POLICY_MAX_WIDTH 512
typedef struct BgPolicyLayer {
  const void* weight_dev;  /* bfloat16 [out_features, in_features] */
  const float* bias_dev;   /* float32 [out_features] */
  uint32_t weight_stride_elems;
  uint16_t in_features, out_features;
  uint32_t activation;     /* BG_POLICY_ACT_* */
  uint32_t reserved;       /* 0 */
} BgPolicyLayer;
typedef struct BgPolicyNet {
  uint32_t n_trunk, n_pi, n_vf, has_value, in0, reserved[3];
  BgPolicyLayer layer[BG_POLICY_MAX_LAYERS];
} BgPolicyNet;
int bg_policy_check(const BgPolicyNet* net);
int bg_policy_tap_cols(const BgPolicyNet* net); /* the sum of the hidden widths, or BG_E_ARG */
int bg_policy_forward(const BgPolicyNet* net, const void* h_dev, uint64_t h_stride_elems, const int8_t* mask_dev /*nullable*/, uint64_t mask_stride_bytes,
                      int64_t m, uint32_t flags, uint64_t seed, uint64_t index0, uint64_t t, int32_t* actions_dev, float* log_prob_dev /*nullable*/,
                      float* entropy_dev /*nullable*/, float* values_dev /*nullable*/, void* taps_dev /*nullable*/, uint64_t taps_stride_elems,
                      float* logits_out_dev /*nullable*/, uint64_t logits_out_stride_elems, float* kernel_ms_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
