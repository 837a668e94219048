"""Worker of tests/test_obs_filter_job_gpu.py: ONE rank of a job that synchronises its observation filter through a process group.

    python tests/obs_filter_job_worker.py <rank> <world> <port> <out_dir>

This rank's shard of JOB_ENVS global envs (sharding.make_sharded_env), one policy from POLICY_SEED, an ``ObsFilter(job=True)`` bound
to the env; ROUNDS rounds of {rollout of K steps, ``sync()``}.  Saves, per round, the buffer this rank contributed and the state
after the synchronisation.  Backend: gloo with every rank on cuda:0, the rows staged through host memory (sharding._through_host).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOB_ENVS, K, ROUNDS, POLICY_SEED, ROLLOUT_SEED, HIDDEN = 557, 3, 2, 3, 5, 16


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from ship_sim_gym_amd import sharding
    from ship_sim_gym_amd.obs_filter import ObsFilter
    from ppo_reference import actor_critic_policy
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    env = sharding.make_sharded_env(JOB_ENVS, rank=rank, world_size=world, device=dev, n_maps=16)
    _, pol = actor_critic_policy(torch, env.states_history, HIDDEN, 2, "tanh", 3, seed=POLICY_SEED, device=dev)
    flt = ObsFilter(env, job=True)
    env.set_obs_filter(flt)
    env.reset_tensor()
    buffers, states = [], []
    for r in range(ROUNDS):
        env.rollout_policy(pol, K, seed=ROLLOUT_SEED, step0=r * K)
        buffers.append(flt.buffer.detach().cpu().clone())
        flt.sync()
        states.append(flt.state.detach().cpu().clone())
        assert torch.equal(flt.base, flt.state) and not flt.buffer.any()
    torch.cuda.synchronize()
    torch.save({"buffers": buffers, "states": states, "envs": int(env.num_envs), "env_id_base": int(env.env_id_base), "eps": flt.eps,
                "backend": str(dist.get_backend()), "world": dist.get_world_size()}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
    env.close()


if __name__ == "__main__":
    main()
