"""Worker of tests/test_report_job_gpu.py: ONE rank of a data-parallel job that reports its update job-wide.

    python tests/report_job_worker.py <rank> <world> <port> <out_dir>

Runs sharding.make_sharded_env over this rank's range of JOB_ENVS global envs, one policy from POLICY_SEED and a DataParallelPPO with
the extended loss: one rollout of K steps, gae, update(None, EPOCHS, MINIBATCHES, stats=True), then job_report(stats, post=True,
per_shard=True).  Saves the record, this rank's own sum row (report_row after the update, post group on), the stats rows and the rank's
own report().  Backend: nccl (= RCCL) when the node shows at least `world` devices, else gloo with the ranks on cuda:0.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOB_ENVS, K, EPOCHS, MINIBATCHES = 400, 8, 2, 3
POLICY_SEED, ROLLOUT_SEED, PERM_SEED, HIDDEN = 3, 5, 11, 32
TERMS = dict(vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01)


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from ship_sim_gym_amd import sharding
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ppo_reference import actor_critic_policy
    n_dev = torch.cuda.device_count()
    use_rccl = n_dev >= world
    dev = torch.device("cuda", rank if use_rccl else 0)
    torch.cuda.set_device(dev)
    if use_rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    env = sharding.make_sharded_env(JOB_ENVS, rank=rank, world_size=world, device=dev, n_maps=16)
    _, pol = actor_critic_policy(torch, env.states_history, HIDDEN, 2, "tanh", 3, seed=POLICY_SEED, device=dev)
    ppo = DataParallelPPO(pol, env, plan=(K, MINIBATCHES), perm_seed=PERM_SEED, **TERMS)
    env.reset_tensor()
    b = dict(env.rollout_policy(pol, K, seed=ROLLOUT_SEED, step0=0))
    ppo.gae(b)
    st = ppo.update(b, None, EPOCHS, MINIBATCHES, stats=True)
    rec = ppo.job_report(b, stats=st, post=True, per_shard=True)
    row = ppo.report_row(b, post=True)
    own = ppo.report(b, stats=st, post=True)
    torch.cuda.synchronize()
    torch.save({"record": rec, "row": row.cpu(), "stats": st.cpu(), "own": own, "shard_envs": ppo.shard_envs,
                "backend": str(dist.get_backend()), "world": dist.get_world_size()}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
    env.close()


if __name__ == "__main__":
    main()
