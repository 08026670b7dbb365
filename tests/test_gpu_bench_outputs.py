"""bench.py end to end on a small batch: --steps is the number of env steps timed, and --dump-outputs
writes what the last timed step handed its caller — checked against an independent spl_step chain of
the same seeds over the warm-up and the timed steps (the library's own rollout == step-chain property,
tests/test_gpu_parity.py, through the benchmark's launch loop: whole launches, a shorter last launch,
graph replays with an eager tail)."""
import json
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

T = 1024
NAMES = ("obs", "mask", "reward", "terminated", "flags", "winner")


def run_bench(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("mode,steps", [("rollout", 20), ("rollout", 300), ("step", 100), ("step", 20)])
def test_dumped_outputs_equal_a_step_chain(mode, steps, tmp_path, monkeypatch, capsys):
    """20 steps: one short rollout launch; 300: two 128-step launches and one of 44; step mode, 100: one
    64-step graph replay and 36 eager launches; step mode, 20: eager launches only."""
    import torch
    from splendor_gym.device import Engine
    out = run_bench(monkeypatch, capsys, "--gpus", "1", "--steps", str(steps), "--warmup", "5", "--tables", str(T),
                    "--mode", mode, "--dump-outputs", str(tmp_path))
    assert out["steps"] == steps and out["config"]["requested_steps"] == steps
    assert out["ms_per_step"] > 0
    # value = tables x steps / timed seconds, ms_per_step = timed seconds / steps (both rounded in the line)
    assert out["value"] == pytest.approx(T / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert out["error_flags"] == 0 and out["launch_faults"] == 0
    assert "cpu_baseline" in out and out["cpu_baseline"] is None  # a plain run measures the headline alone
    for key in ("other_mode", "in_place_l3", "rollout_store", "config5_selfplay", "config4_share", "caller_path"):
        assert key not in out
    plan = bench.headline_plan(mode, steps, 5, bench.REFILL_EVERY[2])
    assert out["warmup"] == plan["W"]

    chain = Engine(T, 2, refill_period=bench.REFILL_EVERY[2])
    chain.reset(seeds=range(T))
    dev = chain.device
    a = torch.zeros(T, dtype=torch.int32, device=dev)
    chain.sample_uniform(out=a, seed=0, ply=0)
    ep_ret = torch.zeros(T, dtype=torch.float32, device=dev)
    ep_cnt = torch.zeros(T, dtype=torch.int32, device=dev)
    # step mode with graphs: one untimed replay of G steps between the warm-up and the timed region
    for i in range(plan["W"] + plan["G"] + steps):
        na = torch.empty_like(a)
        chain.step(a, next_actions=na, policy_seed=0, ply=1 + i, ep_return=ep_ret, ep_count=ep_cnt)
        a = na
    want = {name: getattr(chain, name) for name in NAMES}
    want["final_obs"] = chain.final_obs * chain.terminated.bool().unsqueeze(1)
    want.update(next_actions=a, ep_return=ep_ret, ep_count=ep_cnt)
    # random 2-player games last ~77 plies and the shortest case runs 84: episodes ended and were re-dealt on the way
    assert int(ep_cnt.sum()) > T // 4
    total = 0
    tables = np.load(tmp_path / "tables.npy")
    assert tables.dtype == np.float64 and np.array_equal(tables, np.arange(T))
    for name, t in want.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32, name
        total += got.nbytes
        np.testing.assert_array_equal(got, t.to(torch.float32).cpu().numpy(), err_msg=name)
    assert total + tables.nbytes <= 64 << 20
    chain.close()
