"""What tests/test_adv_norm_job_gpu.py and its worker share: a job of W shards replayed in ONE process over the public halves of
DataParallelPPO(job_adv_norm="minibatch") with torch.stack as the gather, and the checksum both print.  No fixtures, no device code."""
import hashlib

K, EPOCHS, MINIBATCHES = 8, 2, 3
POLICY_SEED, ROLLOUT_SEED, PERM_SEED, HIDDEN = 3, 5, 11, 32
TERMS = dict(vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01)
BATCH_KEYS = ("obs", "act", "logp", "val", "rew", "done", "last_val")


def checksum(params, adam_mv, table):
    """sha256 over the parameters, the Adam moments and the last update's table of stats rows."""
    h = hashlib.sha256()
    for t in (params, adam_mv, table):
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def replay_update(torch, trainers, batches, shard_envs):
    """One update of a job whose shard r is trainers[r] (a DataParallelPPO of its own, member r, job_adv_norm="minibatch") over
    batches[r] (rollout dicts on the device; K x shard_envs[r] samples): GAE and the job's moments, the permutations, every shard's
    sums, the stack as the gather, the same table on every shard, then per minibatch the select, the local rows and the apply.
    Returns (the stacked sums f64 [W, epochs * chunks, 4], the job's stats rows)."""
    from ship_sim_gym_amd.dp import chunk_counts
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    moments, perms, sums = [], [], []
    for tr, b in zip(trainers, batches):
        NativePPO.gae(tr, b)
        moments.append(tr.shard_moments(b))
    for tr, b in zip(trainers, batches):
        tr.set_moments(torch.stack(moments))
        tr.dist(b)  # (from the parameters on entry, as update() takes it)
        perms.append(tr.draw_perm(b, EPOCHS))
        sums.append(tr.shard_minibatch_sums(b, perms[-1], MINIBATCHES))
    stacked = torch.stack(sums)
    for tr in trainers:
        tr.set_minibatch_rows(stacked)
    chunks = [chunk_split(K * e, MINIBATCHES) for e in shard_envs]
    n_chunks = chunks[0][1]
    assert all(c[1] == n_chunks for c in chunks)
    stats = []
    for e in range(EPOCHS):
        for j in range(n_chunks):
            rows = []
            for tr, b, perm, (chunk, _) in zip(trainers, batches, perms, chunks):
                tr.select_minibatch(e, j)
                rows.append(tr.local_row(b, perm[e, j * chunk: (j + 1) * chunk]))
            rows = torch.stack(rows)
            for tr in trainers:
                st = tr.apply_rows(rows, chunk_counts(K, shard_envs, MINIBATCHES, j), j == 0, e == EPOCHS - 1 and j == n_chunks - 1, stats=True)
            stats.append(st)
    for tr in trainers:
        tr.updates += 1
    return stacked, torch.stack(stats)
