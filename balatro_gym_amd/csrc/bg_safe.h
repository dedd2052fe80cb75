// bg_safe.h -- SafeBalatroEnv's episode limits (train_balatro_fixed.py:228-277), the rule of one step of one env, for bg_step_many_rows_ex.
//
// Every training script of the reference wraps the env as Monitor(SafeBalatroEnv(BalatroEnvFixed(seed + rank), max_invalid_actions=50,
// max_episode_steps=1000)).  The wrapper keeps two counters per env -- steps of the episode, consecutive rewards of exactly -1.0 -- and ends the
// episode when either reaches its limit: the invalid-action limit with reward -50.0 and terminated, the step limit with truncated.  The rule is plain
// C++ behind BG_SAFE_FN, so the text the owner lanes of bg_engine3.h run compiles with g++ (define BG_SAFE_HOST before including; the pattern of
// bg_gae.h / bg_head.h): tests/test_step_many_safe_host.py holds it to the reference's own wrapper output, tests/golden/sb3_fixed.npz.
#ifndef BG_SAFE_H
#define BG_SAFE_H
#include <stdint.h>

#ifdef BG_SAFE_HOST
#define BG_SAFE_FN static inline
#else
#define BG_SAFE_FN __host__ __device__ __forceinline__
#endif

// the bits of a record's byte BG_ROW_END_FLAGS: include/balatro_mi355x.h's BG_END_GAME / BG_END_INVALID / BG_END_MAX_STEPS under names of this header's
// own, so that it compiles alone (bg_lib.hip asserts that the two sets agree)
#define BG_SAFE_END_GAME 1u
#define BG_SAFE_END_INVALID 2u
#define BG_SAFE_END_MAX_STEPS 4u
#define BG_SAFE_MIN_LIMIT 3          // both limits: see bg_step_many_rows_ex (the ring arithmetic of bg_chunk_limit)
#define BG_SAFE_KILL_REWARD (-50.0)  // :249

struct BgSafeStep {
  int32_t episode_steps, consecutive_invalid;   // the counters behind the step (both 0 when it ended the episode: reset(), :271-277)
  double reward;                                // the reward to record: -50.0 on a kill, the step's own otherwise
  uint32_t flags;                               // BG_SAFE_END_* (= BG_END_*) bits; non-zero exactly when the step ended the episode (SB3's done)
};

// One step (:239-260).  `reward` / `env_terminated`: what the env's own step returned.  The test is on the reward's VALUE, exactly -1.0 in float64:
// an invalid action, and a consumable that failed (BG_ERR_CONSUMABLE*), as in the reference.
BG_SAFE_FN BgSafeStep bg_safe_step(double reward, bool env_terminated, int32_t episode_steps, int32_t consecutive_invalid,
                                   int32_t max_invalid_actions, int32_t max_episode_steps) {
  BgSafeStep o;
  episode_steps += 1;                                              // :242
  bool kill = false;
  if (reward == -1.0 && !env_terminated) {                         // :245 (the env never sets truncated)
    consecutive_invalid += 1;
    if (consecutive_invalid >= max_invalid_actions) { kill = true; reward = BG_SAFE_KILL_REWARD; }   // :247-250
  } else {
    consecutive_invalid = 0;                                       // :252
  }
  const bool max_steps = episode_steps >= max_episode_steps;       // :255
  o.flags = (env_terminated ? BG_SAFE_END_GAME : 0u) | (kill ? BG_SAFE_END_INVALID : 0u) | (max_steps ? BG_SAFE_END_MAX_STEPS : 0u);
  o.reward = reward;
  o.episode_steps = o.flags ? 0 : episode_steps;
  o.consecutive_invalid = o.flags ? 0 : consecutive_invalid;
  return o;
}
// an ending the WRAPPER made: the env itself did not terminate, so it has not been reset yet
BG_SAFE_FN bool bg_safe_wrapper_ending(uint32_t flags) { return flags != 0u && !(flags & BG_SAFE_END_GAME); }
// terminal slots a call of K steps can use per env: its first wrapper ending may come at step 0 (the counters are carried in), every further one
// needs min(limits) more steps
BG_SAFE_FN int32_t bg_safe_slots(int32_t K, int32_t max_invalid_actions, int32_t max_episode_steps) {
  const int32_t m = max_invalid_actions < max_episode_steps ? max_invalid_actions : max_episode_steps;
  return m < 1 || K < 0 ? -1 : K / m + 1;
}
#endif
