"""Worker of tests/test_episode_log_job_gpu.py: ONE rank of a data-parallel job that keeps the job's episode log.

    python tests/episode_log_job_worker.py <rank> <world> <port> <out_dir>

Makes a handle over this rank's range of JOB_ENVS global envs (the handle serves the calls only: the batches are synthetic, this rank's
columns of episode_log_job_support.inputs over all the job's envs) and an ``EpisodeLog(job=True)`` whose job size and total env count
come from the process group, and calls ``job_append`` on CALLS batches.  Saves the ring, the head, this rank's carries and each call's
own block.  Backend: nccl (= RCCL) when the node shows at least `world` devices, else gloo with the ranks on cuda:0.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOB_ENVS, ROWS, CAPACITY = 321, 5, 97
CALLS = ((5, "p0.3", 21), (3, "p1", 22), (5, "last_row", 23))  # (K, pattern, seed)


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from ship_sim_gym_amd.episode_log import EpisodeLog
    from ship_sim_gym_amd.sharding import shard_range
    from episode_log_job_support import inputs
    from gpu_support import vec
    n_dev = torch.cuda.device_count()
    use_rccl = n_dev >= world
    dev = torch.device("cuda", rank if use_rccl else 0)
    torch.cuda.set_device(dev)
    if use_rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_range(JOB_ENVS, rank, world)
    env = vec(hi - lo, 7, base=lo)
    log = EpisodeLog(env, capacity=CAPACITY, job=True, rows=ROWS)
    log.ring.fill_(0xAB)
    blocks = []
    for K, pattern, seed in CALLS:
        rew, done, flags = (torch.from_numpy(a[:, lo:hi].copy()).to(dev) for a in inputs(K, JOB_ENVS, pattern, seed))
        batch = {"rew": rew, "done": done, "flags": flags}
        mine = EpisodeLog(env, capacity=CAPACITY, job=True, rows=ROWS, world=world, total_envs=JOB_ENVS)  # this call's own block, for the replay
        mine.carry_return.copy_(log.carry_return)
        mine.carry.copy_(log.carry)
        mine.steps = log.steps
        blocks.append(mine.shard_block(batch).cpu())
        log.job_append(batch)
    torch.cuda.synchronize()
    torch.save({"ring": log.ring.cpu(), "head": log.head.cpu(), "carry_return": log.carry_return.cpu(), "carry": log.carry.cpu(),
                "blocks": torch.stack(blocks), "world": log.world, "total_envs": log.total_envs, "stage": log.stage, "steps": log.steps,
                "backend": str(dist.get_backend())}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
    env.close()


if __name__ == "__main__":
    main()
