// bg_progress.h -- ProgressionRewardWrapper's reward shaping (train_progressive.py:21-120), the rule of one step of one env, for
// bg_step_many_rows_progress.
//
// The reference's most recent training script wraps the env as Monitor(SafeBalatroEnv(ProgressionRewardWrapper(BalatroEnvFixed(seed + rank)),
// max_invalid_actions=50, max_episode_steps=1000)) (train_progressive.py:123-131).  The wrapper sits INSIDE SafeBalatroEnv: it adds bonuses for new
// antes and rounds and penalties for staying on ante 1 to the env's reward, and ends the episode itself -- terminated, 50 off the reward -- after more
// than 300 steps on ante 1; SafeBalatroEnv's `reward == -1.0` test (bg_safe.h) then reads the SHAPED reward.  The rule is plain C++ behind
// BG_PROGRESS_FN, so the text the owner lanes of bg_engine3.h run compiles with g++ (define BG_PROGRESS_HOST before including; the pattern of
// bg_safe.h): tests/test_step_many_progress_host.py holds it to the reference's own wrapper output, tests/golden/progression.npz.
#ifndef BG_PROGRESS_H
#define BG_PROGRESS_H
#include <stdint.h>

#ifdef BG_PROGRESS_HOST
#define BG_PROGRESS_FN static inline
#else
#define BG_PROGRESS_FN __host__ __device__ __forceinline__
#endif

// the bit of a record's byte BG_ROW_END_FLAGS: include/balatro_mi355x.h's BG_END_STUCK under a name of this header's own, so that it compiles alone
// (bg_lib.hip asserts that the two agree)
#define BG_PROGRESS_END_STUCK 8u
#define BG_PROGRESS_STUCK_STEPS 300   // :96: more steps than this on ante 1 end the episode, i.e. step 301 at the earliest

// The wrapper's state (:27-31), and after reset() (:33-41): total_steps 0, steps_on_current_ante 0, last_ante / last_round / max_ante_reached 1.
struct BgProgressCarry {
  int32_t total_steps, steps_on_current_ante, last_ante, last_round, max_ante_reached;
};
// As the caller keeps it: int32 [N, 4], an all-zero row = the state after reset().
//   word 0: total_steps            0 .. 2**31 - 1   (reset by every ending; with limits at most max_episode_steps)
//   word 1: steps_on_current_ante  0 .. 2**31 - 1   (<= total_steps)
//   word 2: (last_ante - 1) | (max_ante_reached - 1) << 16: both 1 .. 65536.  Both only ever take a value of state.ante above 1, and the engine keeps
//           state.ante in one byte (bg_pack; the game ends above ante 100, an injected level is a byte too), so 1 .. 255 occur.
//   word 3: last_round - 1, the whole int32: state.round is 1 .. 3 (a byte in bg_pack), and :118 may copy any value of it.
struct BgProgressPacked { int32_t w[4]; };
BG_PROGRESS_FN BgProgressPacked bg_progress_pack(const BgProgressCarry& c) {
  BgProgressPacked p;
  p.w[0] = c.total_steps; p.w[1] = c.steps_on_current_ante;
  p.w[2] = (int32_t)(((uint32_t)(c.last_ante - 1) & 0xffffu) | (((uint32_t)(c.max_ante_reached - 1) & 0xffffu) << 16));
  p.w[3] = c.last_round - 1;
  return p;
}
BG_PROGRESS_FN BgProgressCarry bg_progress_unpack(const BgProgressPacked& p) {
  BgProgressCarry c;
  c.total_steps = p.w[0]; c.steps_on_current_ante = p.w[1];
  c.last_ante = (int32_t)((uint32_t)p.w[2] & 0xffffu) + 1; c.max_ante_reached = (int32_t)((uint32_t)p.w[2] >> 16) + 1;
  c.last_round = p.w[3] + 1;
  return c;
}

struct BgProgressStep {
  BgProgressCarry carry;   // the state behind the step (NOT reset on `stuck`: the caller resets it with every ending, whoever made it)
  double reward;           // the shaped reward
  bool stuck;              // the wrapper's own terminated = True (:97, info['stuck_on_ante_1'])
};

// One step (:43-120).  `reward`: what the env's own step returned; `ante` / `round`: state.ante / state.round behind that step (:50-57) -- of the
// FINAL state when the step ended the game.  Every float64 addition is the reference's, in its order, one rounding each (build with
// -ffp-contract=off: nothing here may become an FMA).
BG_PROGRESS_FN BgProgressStep bg_progress_step(double reward, int32_t ante, int32_t round, BgProgressCarry c) {
  BgProgressStep o;
  o.stuck = false;
  c.total_steps += 1;                                                       // :45
  if (ante == c.last_ante) c.steps_on_current_ante += 1;                    // :60-61
  else c.steps_on_current_ante = 0;                                         // :62-63
  if (ante > c.last_ante) {                                                 // :66
    reward += (double)(200 * (ante - c.last_ante));                         // :68-69
    c.last_ante = ante;                                                     // :72
  }
  if (round > c.last_round && ante == c.last_ante) {                        // :75
    reward += 20.0;                                                         // :76-77
    c.last_round = round;                                                   // :78
  }
  if (ante > c.max_ante_reached) {                                          // :81
    c.max_ante_reached = ante;                                              // :82
    reward += 100.0;                                                        // :84-85
  }
  if (ante == 1 && c.steps_on_current_ante > 150) {                         // :91
    reward += -0.5 * (double)(c.steps_on_current_ante - 150);               // :92-93
    if (c.steps_on_current_ante > BG_PROGRESS_STUCK_STEPS) {                // :96
      o.stuck = true;                                                       // :97
      reward -= 50.0;                                                       // :98
    }
  }
  if (c.total_steps > 200 && ante < 2) reward -= 0.2;                       // :103-104
  else if (c.total_steps > 400 && ante < 3) reward -= 0.3;                  // :105-106
  else if (c.total_steps > 600 && ante < 4) reward -= 0.4;                  // :107-108
  if (ante >= 3 && c.total_steps < 300) reward += 50.0;                     // :111-113 (every such step)
  if (ante != c.last_ante) c.last_round = round;                            // :117-118 (only below last_ante: an ante above it was taken at :72)
  o.carry = c;
  o.reward = reward;
  return o;
}
// terminal slots a call of K steps can use per env under both wrappers: the first wrapper ending may come at step 0 (the state is carried in), every
// further one needs min(max_invalid_actions, max_episode_steps, 301) more steps (a stuck ending needs 301 steps on ante 1)
BG_PROGRESS_FN int32_t bg_progress_slots(int32_t K, int32_t max_invalid_actions, int32_t max_episode_steps) {
  int32_t m = max_invalid_actions < max_episode_steps ? max_invalid_actions : max_episode_steps;
  if (m > BG_PROGRESS_STUCK_STEPS + 1) m = BG_PROGRESS_STUCK_STEPS + 1;
  return m < 1 || K < 0 ? -1 : K / m + 1;
}
#endif
