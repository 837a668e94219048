"""Worker of tests/test_adv_norm_job_gpu.py: ONE rank of a data-parallel job with job_adv_norm="minibatch" on the product path.

    python tests/adv_norm_job_worker.py <rank> <world> <port> <out_dir>

Runs sharding.make_sharded_env over this rank's range of JOB_ENVS global envs, one policy from POLICY_SEED and a
DataParallelPPO(job_adv_norm="minibatch") with the extended loss, then ROUNDS rounds of {rollout of K steps, gae, update(None, EPOCHS,
MINIBATCHES)}.  Prints the checksum of the parameters, the moments and the last table, and saves every round's batch.  Backend: nccl
(= RCCL) when the node shows at least `world` devices, else gloo with the ranks on cuda:0 (tests/dp_worker.py's rule).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOB_ENVS, ROUNDS = 192, 2


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    import adv_norm_job_support as S
    from ship_sim_gym_amd import sharding
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ppo_reference import actor_critic_policy
    use_rccl = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if use_rccl else 0)
    torch.cuda.set_device(dev)
    if use_rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    env = sharding.make_sharded_env(JOB_ENVS, rank=rank, world_size=world, device=dev, n_maps=16)
    _, pol = actor_critic_policy(torch, env.states_history, S.HIDDEN, 2, "tanh", 3, seed=S.POLICY_SEED, device=dev)
    ppo = DataParallelPPO(pol, env, plan=(S.K, S.MINIBATCHES), perm_seed=S.PERM_SEED, job_adv_norm="minibatch", **S.TERMS)
    assert (ppo.rank, ppo.world, ppo.member) == (rank, world, rank) and sum(ppo.shard_envs) == JOB_ENVS
    env.reset_tensor()
    batches, stats = [], []
    for r in range(ROUNDS):
        b = dict(env.rollout_policy(pol, S.K, seed=S.ROLLOUT_SEED, step0=r * S.K))
        batches.append({k: b[k].detach().cpu().clone() for k in S.BATCH_KEYS})
        ppo.gae(b)
        stats.append(ppo.update(b, None, S.EPOCHS, S.MINIBATCHES, stats=True).cpu())
    torch.cuda.synchronize()
    torch.save({"batches": batches, "stats": stats, "shard_envs": ppo.shard_envs, "step": ppo.step}, os.path.join(out_dir, "rank%d.pt" % rank))
    print("checksum %s" % S.checksum(pol.params, ppo.adam_mv, ppo.minibatch_table()), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    env.close()


if __name__ == "__main__":
    main()
