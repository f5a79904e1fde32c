"""GPU box, 2 and 4 ranks sharing the one MI355X (gloo carries the collectives; the 8-GPU runs use RCCL through the
same code; the box admits 6 GPU processes, the test runner being one of them): the sharded CEM rollouts reproduce the
single-rank costs and elite set -- ragged shards, `opt_traj` on the last rank, the un-sharded debug outputs -- and the
data-parallel train step leaves every rank with the mean of the per-rank gradients."""
import argparse
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

FLAGS = dict(model_use_mask=False, model_use_future_mask=False, model_use_robot_state=False, reconstruction_loss="l1")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ns(dev, **kw):
    from oracle import svg_oracle as orc
    cfg = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, n_past=1, n_future=2, lr=1e-4, candidates_batch_size=4,
                  sample_mean=True, reward_type="dense", topk=3, **FLAGS)
    d = dict(cfg.__dict__)
    d.update(device=dev, debug_cem=False, log_dir="/tmp/rac_dist", img_cost_threshold=None, img_cost_world_norm=True,
             experiment="train_robonet", robot_joint_dim=5, load_movement_info=False, movement_weight=1.0,
             scheduled_sampling=False, scheduled_sampling_k=4000, model="svg", optimizer="adam", seed=0, wandb=False,
             cem_shard=True, ddp_bucket_mb=1, dynamics_model_ckpt=None)
    d.update(kw)
    return cfg, argparse.Namespace(**d)


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0")
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from oracle import svg_oracle as orc
        from robot_aware_control_amd import synthetic as syn
        from robot_aware_control_amd import trainer as trainer_mod
        from robot_aware_control_amd.cem import CEMPolicy
        from robot_aware_control_amd.model import SVGConvModel
        from robot_aware_control_amd.state import DemoGoalState, State
        from robot_aware_control_amd.trainer import PredictionTrainer
        out = {"rank": rank}

        # ---- sharded CEM: 11 candidates over 2 ranks (ragged shards, batch 4) ----
        cfg, ns = _ns(dev)
        sd = orc.make_weights(cfg, seed=9, action_gain=200.0)
        model = SVGConvModel(ns)
        model.load_state_dict({k: v.clone() for k, v in sd.items()})
        model.eval()
        N, T = 11, 4
        prob = syn.synth_cem_problem(seed=5, N=N, T=T, goal_blend=0.15)
        start, goal = State(img=prob["start_img"]), DemoGoalState(imgs=prob["goal_imgs"], masks=prob["goal_masks"])
        pol = CEMPolicy(ns, model, horizon=T + 1, opt_iter=2, action_candidates=N, topk=3, init_std=0.03)
        opt = prob["actions"][0, :, :2].clone() * 0.5
        ro_sh = pol.traj_sampler.generate_model_rollouts(prob["actions"].clone(), start, goal, opt_traj=opt.clone())
        dbg_sh = pol.traj_sampler.generate_model_rollouts(prob["actions"].clone(), start, goal, ret_obs=True,
                                                          ret_step_cost=True)
        ns.cem_shard = False
        ro_1 = pol.traj_sampler.generate_model_rollouts(prob["actions"].clone(), start, goal, opt_traj=opt.clone())
        dbg_1 = pol.traj_sampler.generate_model_rollouts(prob["actions"].clone(), start, goal, ret_obs=True,
                                                         ret_step_cost=True)
        ns.cem_shard = True
        # per-candidate math is batch-independent by construction (eval BN; the frozen model's split-precision convs take
        # one operand scale per image and never split K): sharded == single rank bit for bit, opt_traj included
        out["cem_equal"] = bool(np.array_equal(ro_sh["sum_cost"], ro_1["sum_cost"])
                                and ro_sh["optimal_sum_cost"] == ro_1["optimal_sum_cost"])
        out["debug_equal"] = bool(np.array_equal(dbg_sh["obs"], dbg_1["obs"]) and np.array_equal(dbg_sh["step_cost"], dbg_1["step_cost"])
                                  and list(dbg_sh["topk_idx"]) == list(dbg_1["topk_idx"]) and np.abs(dbg_sh["obs"]).max() > 0)
        out["dbg"] = [float(np.abs(dbg_sh["obs"] - dbg_1["obs"]).max()),
                      float(np.abs(dbg_sh["step_cost"] - dbg_1["step_cost"]).max() / np.abs(dbg_1["step_cost"]).max()),
                      [int(i) for i in dbg_sh["topk_idx"]], [int(i) for i in dbg_1["topk_idx"]]]
        # ---- robot-aware planner: sharded BEFORE the robot model is asked (a rank asks about ITS candidates only) ----
        from robot_aware_control_amd.trajectory_sampler import TrajectorySampler, shard_bounds
        ra_flags = dict(model_use_mask=True, model_use_future_mask=True, model_use_robot_state=True,
                        reconstruction_loss="dontcare_l1")
        cfg_ra = orc.Cfg(g_dim=64, z_dim=16, batch_size=2, candidates_batch_size=4, sample_mean=True,
                         reward_type="dontcare", topk=3, **ra_flags)
        _, ns_ra = _ns(dev, reward_type="dontcare", experiment="control_wx250s_synthetic", **ra_flags)
        m_ra = SVGConvModel(ns_ra)
        m_ra.load_state_dict({k: v.clone() for k, v in orc.make_weights(cfg_ra, seed=9, action_gain=200.0).items()})
        m_ra.eval()

        class Counting:  # the atlas robot model, recording how many candidates each call asked about
            def __init__(self, inner):
                self.inner, self.asked, self.shared_start_mask = inner, [], None

            def predict_batch(self, data, thick=True):
                self.asked.append(int(data["actions"].shape[1]))
                res = self.inner.predict_batch(data, thick)
                self.shared_start_mask = self.inner.shared_start_mask
                return res
        robot = Counting(syn.SyntheticArmModel(dev).atlas(54, 61))
        s_ra = State(img=prob["start_img"], state=np.array([0.28, 0.0, 0.12, 0.0, 0.0], np.float32),
                     qpos=np.zeros(5, np.float32))
        g_ra = DemoGoalState(imgs=prob["goal_imgs"], masks=[np.zeros((1, 64, 64), bool)])
        smp = TrajectorySampler(ns_ra, m_ra, robot_model=robot)
        ra_sh = smp.generate_model_rollouts(prob["actions"].clone(), s_ra, g_ra, opt_traj=opt.clone())
        lo_, hi_ = shard_bounds(N + 1, world, rank)
        out["ra_asked_local"] = robot.asked == [hi_ - lo_] and robot.shared_start_mask is True
        ns_ra.cem_shard = False
        ra_1 = smp.generate_model_rollouts(prob["actions"].clone(), s_ra, g_ra, opt_traj=opt.clone())
        ns_ra.cem_shard = True
        out["ra_equal"] = bool(np.array_equal(ra_sh["sum_cost"], ra_1["sum_cost"]) and robot.asked[-1] == N + 1
                               and ra_sh["optimal_sum_cost"] == ra_1["optimal_sum_cost"]
                               and np.unique(ra_1["sum_cost"]).size > N // 2)
        del m_ra, smp
        # the same at the benchmarked width (g 512 / z 64): 37 candidates in ragged shards and batches of 8 against one
        # un-sharded pass of all 37 -- per-image operand scales and an unsplit K make a cost independent of its batch
        cfg5, ns5 = _ns(dev, g_dim=512, z_dim=64, candidates_batch_size=8)
        cfg5.g_dim, cfg5.z_dim = 512, 64
        big = SVGConvModel(ns5)
        big.load_state_dict({k: v.clone() for k, v in orc.make_weights(cfg5, seed=9, action_gain=200.0).items()})
        big.eval()
        prob5 = syn.synth_cem_problem(seed=6, N=37, T=3, goal_blend=0.15)
        pol5 = CEMPolicy(ns5, big, horizon=4, opt_iter=1, action_candidates=37, topk=5, init_std=0.03)
        s5, g5 = State(img=prob5["start_img"]), DemoGoalState(imgs=prob5["goal_imgs"], masks=prob5["goal_masks"])
        c_sh = pol5.traj_sampler.generate_model_rollouts(prob5["actions"].clone(), s5, g5)["sum_cost"]
        ns5.cem_shard, ns5.candidates_batch_size = False, 37
        c_1 = pol5.traj_sampler.generate_model_rollouts(prob5["actions"].clone(), s5, g5)["sum_cost"]
        out["g512_equal"] = bool(np.array_equal(c_sh, c_1) and np.unique(c_1).size > 30)
        del big, pol5
        torch.cuda.empty_cache()
        torch.manual_seed(100 + rank)  # different RNG per rank: the candidate draw must still agree (rank-0 broadcast)
        out["action"] = pol.get_action(start, goal, 0, 0).tolist()

        # ---- data-parallel train step ----
        tr = PredictionTrainer(ns)
        tr.model.load_state_dict({k: v.clone() for k, v in orc.make_weights(cfg, seed=1, randomize_bn_stats=False).items()})
        tr.model.train()
        tr.model.eps_source = lambda shape: torch.zeros(shape)
        tr.optimizer.step = lambda: None
        data = syn.synth_video(seed=30 + rank, T=3, B=2)
        real = trainer_mod._dist_on
        trainer_mod._dist_on = lambda: False  # local gradients only
        tr._train_step(data)
        local = tr.model.flat_parameters()[1].clone()
        parts = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(parts, local)
        mean = sum(parts) / world
        trainer_mod._dist_on = real  # GradReducer: LSTM slices as their wgrads finish, the rest at the end
        tr.model.load_state_dict({k: v.clone() for k, v in orc.make_weights(cfg, seed=1, randomize_bn_stats=False).items()})
        tr._train_step(data)
        got = tr.model.flat_parameters()[1].clone()
        out["ddp_err"] = float((got - mean).norm() / mean.norm())
        # ... and of a window that feeds its predicted frame back (the per-step path: every weight's time-batched gradient
        # launch -- and, behind it, the slice's all-reduce -- starts when its last step is recorded)
        feedback = [True, True, False]
        trainer_mod._dist_on = lambda: False
        tr.model.load_state_dict({k: v.clone() for k, v in orc.make_weights(cfg, seed=1, randomize_bn_stats=False).items()})
        tr._train_step(data, use_truth=feedback)
        local = tr.model.flat_parameters()[1].clone()
        parts = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(parts, local)
        mean = sum(parts) / world
        trainer_mod._dist_on = real
        tr.model.load_state_dict({k: v.clone() for k, v in orc.make_weights(cfg, seed=1, randomize_bn_stats=False).items()})
        tr._train_step(data, use_truth=feedback)
        got = tr.model.flat_parameters()[1].clone()
        out["ddp_err_fed_back"] = float((got - mean).norm() / mean.norm())

        q.put(out)
        dist.destroy_process_group()
    except Exception as e:  # surface the failure in the parent
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
        raise


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_sharing_one_gpu(world):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert "error" not in r, r.get("error")
    assert all(r["cem_equal"] and r["debug_equal"] for r in res), [(r["cem_equal"], r["debug_equal"], r["dbg"]) for r in res]
    assert all(r["g512_equal"] for r in res)
    # robot-aware: each rank asked its robot model about its own shard only, and the costs are the single-rank bits
    assert all(r["ra_asked_local"] and r["ra_equal"] for r in res), [(r["ra_asked_local"], r["ra_equal"]) for r in res]
    assert all(r["action"] == res[0]["action"] for r in res)
    # identical inputs exclude slope flips; what is left is the all-reduce's summation order
    assert all(r["ddp_err"] < 1e-5 for r in res), res
    assert all(r["ddp_err_fed_back"] < 1e-5 for r in res), res


def test_bench_two_ranks_rehearsal():
    """Plain `python bench.py --gpus 2` end to end (no WORLD_SIZE in the environment: the script starts its own ranks as a
    child torch.distributed.run before it touches the GPU -- the same launch the driver's explicit torchrun command ends
    in), before an 8-GPU node ever runs it: both ranks share this box's one MI355X and gloo stands in for RCCL
    (RAC_BENCH_ONE_GPU / RAC_DIST_BACKEND, the script's own rehearsal switches).  Both gradient-exchange modes are timed
    (--full: a plain run times the headline alone)."""
    import json
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RAC_DIST_BACKEND="gloo", RAC_BENCH_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--cem-candidates", "64", "--cem-batch", "64", "--cem-iters", "1", "--cem-opt-iter", "2",
           "--no-exact", "--no-side", "--full"]  # (the exact-fp32 and configs[4] legs: rank-agnostic, rehearsed in test_gpu_nccl.py)
    res = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]  # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["parallelism"] == "ddp2" and out["config"]["global_batch"] == 32
    assert len(out["ranks"]["train_ms_per_step"]) == 2 and all(v > 0 for v in out["ranks"]["train_ms_per_step"])
    assert out["value"] > 0 and out["roofline"]["frac"] > 0 and "allreduce_exposed" in out["time_breakdown_ms"]
    assert abs(out["per_gpu_value"] * 2 - out["value"]) < 1e-6 * out["value"] and out["efficiency_vs_n1"] is None
    modes = out["ddp_modes"]
    assert modes["headline"] == "allreduce" and modes["allreduce"]["ms_per_step"] == out["ms_per_step"]
    assert modes["sharded"].get("ms_per_step", 0) > 0, modes["sharded"]
    assert modes["sharded"]["allreduce_exposed"] is not None and len(modes["sharded"]["rank_ms_per_step"]) == 2
    # each mode line names the optimiser class that really ran (a world size the sharded step cannot cut falls back)
    assert modes["allreduce"]["optimizer"] == "FusedAdam" and modes["sharded"]["optimizer"] == "ShardedAdam"
    assert "fallback" not in modes["sharded"] and out["optimizer"]["optimizer"] == "FusedAdam"
    # what the collective library saw: backend, world size, the card behind every rank
    d = out["dist"]
    assert d["backend"] == "gloo" and d["world_size"] == 2 and [c["rank"] for c in d["devices"]] == [0, 1]
    assert all(c["index"] == 0 and c["name"] for c in d["devices"])  # (the rehearsal: both ranks on this box's one card)
    assert all(isinstance(v, (int, float)) for v in out["time_breakdown_ms"].values())
    cem = out["cem"]
    assert cem["config"]["parallelism"] == "candidate-shard2" and cem["config"]["candidates"] == 128
    assert cem["ranks"]["cost_allgather_ms"] is not None and len(cem["ranks"]["s_per_iteration"]) == 2
    assert out["cem_ra"]["value"] > 0 and "fp32_exact" not in out and "side" not in out
    assert "cpu_baseline" not in out  # rank 0 at N = 1 only
