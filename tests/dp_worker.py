"""Worker of tests/test_dp_gpu.py: ONE rank of a data-parallel training job on the product path.

    python tests/dp_worker.py <rank> <world> <port> <out_dir>

Runs sharding.make_sharded_env over this rank's range of JOB_ENVS global envs, one policy from POLICY_SEED and a DataParallelPPO with
the extended loss, then ROUNDS rounds of {rollout of K steps, gae, update(None, EPOCHS, MINIBATCHES)}.  Saves every round's batch and the
final parameters, moments, KL coefficient and stats rows.  Backend: nccl (= RCCL) when the node shows at least `world` devices, else
gloo with the ranks on cuda:0 and the rows staged through host memory (sharding._through_host) — the 1-GPU test box.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOB_ENVS, K, ROUNDS, EPOCHS, MINIBATCHES = 400, 7, 2, 2, 3
POLICY_SEED, ROLLOUT_SEED, PERM_SEED, HIDDEN = 3, 5, 11, 32
TERMS = dict(vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01)
BATCH_KEYS = ("obs", "act", "logp", "val", "rew", "done", "last_val")


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
    assert (ppo.rank, ppo.world, ppo.member) == (rank, world, rank) and sum(ppo.shard_envs) == JOB_ENVS
    env.reset_tensor()
    batches, stats = [], []
    for r in range(ROUNDS):
        b = dict(env.rollout_policy(pol, K, seed=ROLLOUT_SEED, step0=r * K))
        batches.append({k: b[k].detach().cpu().clone() for k in BATCH_KEYS})
        ppo.gae(b)
        stats.append(ppo.update(b, None, EPOCHS, MINIBATCHES, stats=True).cpu())
    torch.cuda.synchronize()
    torch.save({"batches": batches, "stats": stats, "params": pol.params.detach().cpu(), "adam_mv": ppo.adam_mv.cpu(),
                "kl_coef": ppo.kl_coef.cpu(), "adv_stats": ppo.adv_stats().cpu().clone(), "step": ppo.step, "updates": ppo.updates,
                "shard_envs": ppo.shard_envs, "env_id_base": int(env.env_id_base), "backend": str(dist.get_backend()), "n_dev": n_dev,
                "world": dist.get_world_size()}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()
    env.close()


if __name__ == "__main__":
    main()
