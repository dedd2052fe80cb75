"""numpy restatement of bg_episode_ends_rows (csrc/bg_ends.h): the report over a [K, N] rollout of packed records and the curriculum's rule per
env, CurriculumTracker.update's (sb3_adapter.py:260-279; CurriculumBalatroEnv, train_balatro_agent.py:126-170).  tests/test_episode_ends_host.py
holds it against CurriculumTracker.update itself and against the header compiled for the host; the GPU tests hold the kernel against it."""
import numpy as np

ENDS_WORDS = 32
R_TERM, R_FLAGS, R_END_ANTE, R_END_ROUND, R_END_CHIPS = 342, 343, 344, 346, 348
END_GAME, END_INVALID, END_MAX_STEPS = 1, 2, 4
CAP_MAX = 255


def fields(rows):
    """(terminated uint8, flags uint8, ante int16, round int8, chips uint32), each [K, N], of records [K, N, >= 352]."""
    rows = np.asarray(rows)
    ante = np.ascontiguousarray(rows[:, :, R_END_ANTE:R_END_ANTE + 2]).view(np.int16)[:, :, 0]
    rnd = np.ascontiguousarray(rows[:, :, R_END_ROUND:R_END_ROUND + 1]).view(np.int8)[:, :, 0]
    chips = np.ascontiguousarray(rows[:, :, R_END_CHIPS:R_END_CHIPS + 4]).view(np.uint32)[:, :, 0]
    return rows[:, :, R_TERM], rows[:, :, R_FLAGS], ante, rnd, chips


def put_fields(rows, term, flags, ante, rnd, chips):
    """The inverse: writes the five fields into records [K, N, >= 352]."""
    K, N = term.shape
    rows[:, :, R_TERM] = term
    rows[:, :, R_FLAGS] = flags
    rows[:, :, R_END_ANTE:R_END_ANTE + 2] = np.ascontiguousarray(ante, np.int16).reshape(K, N, 1).view(np.uint8)
    rows[:, :, R_END_ROUND] = np.ascontiguousarray(rnd, np.int8).view(np.uint8)
    rows[:, :, R_END_ROUND + 1] = 0
    rows[:, :, R_END_CHIPS:R_END_CHIPS + 4] = np.ascontiguousarray(chips, np.uint32).reshape(K, N, 1).view(np.uint8)


def report(rows, raised=0):
    """int64 [32]: the report of bg_episode_ends_rows over records [K, N, stride]; word 8 = `raised` (the curriculum's)."""
    term, flags, ante, _, chips = fields(rows)
    ended = term != 0
    fl, an, ch = flags[ended].astype(np.int64), ante[ended].astype(np.int64), chips[ended].astype(np.int64)
    has = an > 0
    out = np.zeros(ENDS_WORDS, np.int64)
    out[0] = int(ended.sum())
    out[1] = int((fl & END_GAME != 0).sum())
    out[2] = int((fl & END_INVALID != 0).sum())
    out[3] = int((fl == END_MAX_STEPS).sum())
    out[4] = int(an[has].sum())
    out[5] = int(an[has].max()) if has.any() else 0
    out[6] = int(ch[has].sum())
    out[7] = int(ch[has].max()) if has.any() else 0
    out[8] = int(raised)
    out[9] = int((~has).sum())
    out[16:32] = np.bincount(np.minimum(an[has], 15), minlength=16)
    return out


class Curriculum:
    """bg_curriculum's state for N envs and the rule of one finished episode of one env."""

    def __init__(self, n, initial_max_ante=3, ante_increment=1, success_threshold=0.8, window=100):
        self.n, self.window, self.inc, self.thr = int(n), int(window), int(ante_increment), float(success_threshold)
        self.cap = np.full(self.n, int(initial_max_ante), np.int32)
        self.hist = np.zeros((self.window, self.n), np.int16)
        self.count = np.zeros(self.n, np.int64)
        self.at_level = np.zeros(self.n, np.int32)

    def episode(self, e, ante):
        """One finished episode of env e.  Returns whether its cap rose."""
        self.hist[int(self.count[e]) % self.window, e] = ante
        self.count[e] += 1
        self.at_level[e] += 1
        if self.at_level[e] >= self.window and self.cap[e] > 0:
            kept = min(int(self.count[e]), self.window)
            reached = int((self.hist[:kept, e].astype(np.int64) >= int(self.cap[e])).sum())
            if reached / float(self.window) >= self.thr:
                self.cap[e] = min(int(self.cap[e]) + self.inc, CAP_MAX)
                self.at_level[e] = 0
                return True
        return False

    def update(self, rows):
        """Every ended record with a summary (end ante > 0) of records [K, N, stride], per env in step order.  Returns raised bool [N]: the caps
        rise inside the call, the envs meet them at the call boundary."""
        term, _, ante, _, _ = fields(rows)
        raised = np.zeros(self.n, bool)
        for t, e in np.argwhere((term != 0) & (ante > 0)):   # (row-major: step order per env)
            raised[e] |= self.episode(int(e), int(ante[t, e]))
        return raised
