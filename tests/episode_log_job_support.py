"""What the job-wide episode log's test modules share (tests/test_episode_log_job.py on the host, tests/test_episode_log_job_gpu.py on the
device): the synthetic [K, N] inputs with tests/test_episode_log_gpu.py's done patterns, the cut of a batch into the ranks' shards, the
numpy side of a replayed job (``shard_block_reference`` per shard, ``merge_blocks_reference`` on the stack) and of the single log it must
equal (``episode_log_reference`` over all envs).  Nothing here needs a device at import."""
import numpy as np

GOAL, ENDS = 0x2, np.array([0x1, 0x4, 0x8, 0x10, 0x1 | 0x4, 0x2 | 0x10], dtype=np.uint8)
PATTERNS = ("p0", "p0.3", "p1", "last_lane", "last_row")
FILL = 0xAB
# (W, N): unequal shards (the remainder goes to the lowest ranks), among them shards of 1, 63, 64, 65 and 257 envs
JOBS = ((1, 1), (1, 65), (2, 3), (2, 127), (3, 191), (3, 770), (8, 15), (8, 517))


def inputs(K, n, pattern, seed):
    """(rew f64, done u8, flags u8) [K, n] in numpy."""
    rng = np.random.RandomState(seed)
    rew = rng.choice([1.0, -1.0, -0.01], size=(K, n))
    if pattern == "last_lane":  # env 255, 511, ... and the last env
        done = np.zeros((K, n), dtype=np.uint8)
        done[:, 255::256] = 1
        done[:, n - 1] = 1
    elif pattern == "last_row":
        done = np.zeros((K, n), dtype=np.uint8)
        done[K - 1] = rng.random_sample(n) < 0.5
        done[K - 1, rng.randint(n)] = 1
    else:
        done = (rng.random_sample((K, n)) < float(pattern[1:])).astype(np.uint8)
    flags = np.where(done != 0, ENDS[rng.randint(0, len(ENDS), size=(K, n))], np.where(rng.random_sample((K, n)) < 0.2, GOAL, 0)).astype(np.uint8)
    return rew, done, flags


def shard_ranges(n, W):
    from ship_sim_gym_amd.sharding import shard_range
    return [shard_range(n, r, W) for r in range(W)]


def shard_sizes(n, W):
    return [hi - lo for lo, hi in shard_ranges(n, W)]


def prime_below(x):
    for p in range(x - 1, 1, -1):
        if all(p % q for q in range(2, int(p ** 0.5) + 1)):
            return p
    return 1


def capacities(count):
    """1, count - 1, count, count + 1 and a prime below count (each at least 1)."""
    return sorted({max(1, c) for c in (1, count - 1, count, count + 1, prime_below(count))})


def filled_ring(cap, fill=FILL):
    from ship_sim_gym_amd.episode_log import RECORD_DTYPE
    return np.full(cap * 32, fill, dtype=np.uint8).view(RECORD_DTYPE).copy()


class Single(object):
    """The numpy side of ONE log over all envs: what episode_log_reference leaves, call after call."""

    def __init__(self, n, cap, env_base=0):
        self.ring, self.head = filled_ring(cap), np.zeros(2, dtype=np.int64)
        self.cret, self.c, self.steps, self.env_base = np.zeros(n), np.zeros((n, 2), dtype=np.int32), 0, env_base

    def append(self, rew, done, flags):
        from ship_sim_gym_amd.episode_log import episode_log_reference
        self.ring, self.head, self.cret, self.c = episode_log_reference(rew, done, flags, self.cret, self.c, self.head, self.ring,
                                                                        step0=self.steps, env_base=self.env_base)
        self.steps += rew.shape[0]
        return self


class Job(object):
    """The numpy side of a W-rank job over n envs: per call shard_block_reference on every shard's columns with its env_base, then
    merge_blocks_reference on the stack.  ``blocks`` keeps the last call's."""

    def __init__(self, n, W, cap, rows, env_base=0):
        from ship_sim_gym_amd.episode_log import job_stage
        self.ranges, self.W, self.rows, self.env_base = shard_ranges(n, W), W, rows, env_base
        self.stage = job_stage(cap, rows, n, W)
        self.ring, self.head = filled_ring(cap), np.zeros(2, dtype=np.int64)
        self.cret = [np.zeros(hi - lo) for lo, hi in self.ranges]
        self.c = [np.zeros((hi - lo, 2), dtype=np.int32) for lo, hi in self.ranges]
        self.steps, self.blocks = 0, None

    def append(self, rew, done, flags):
        from ship_sim_gym_amd.episode_log import merge_blocks_reference, shard_block_reference
        K, blocks = rew.shape[0], []
        for r, (lo, hi) in enumerate(self.ranges):
            b, self.cret[r], self.c[r] = shard_block_reference(rew[:, lo:hi], done[:, lo:hi], flags[:, lo:hi], self.cret[r], self.c[r], self.rows,
                                                               self.stage, step0=self.steps, env_base=self.env_base + lo)
            blocks.append(b)
        self.blocks = np.stack(blocks)
        self.ring, self.head = merge_blocks_reference(self.blocks, self.ring, self.head, K, self.steps, self.rows, self.stage)
        self.steps += K
        return self

    def same_as(self, single, what="", head1=True):
        assert self.ring.tobytes() == single.ring.tobytes(), ("ring", what)
        assert self.head.tolist()[:2 if head1 else 1] == single.head.tolist()[:2 if head1 else 1], ("head", what, self.head, single.head)
        assert np.concatenate(self.cret).tobytes() == single.cret.tobytes(), ("carry_return", what)
        assert np.concatenate(self.c).tobytes() == single.c.tobytes(), ("carry", what)
