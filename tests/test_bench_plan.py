"""bench.py's step plans: the driver's `--steps 20 --warmup 5` (and any other value) must run and
report the steps actually timed (VERDICT r01 "What's weak" 1).  step_plan (the secondary measurements
of --full) rounds up to whole launches; headline_plan (the headline) times --steps exactly."""
import pytest

import bench


@pytest.mark.parametrize("steps", [1, 20, 100, 1024])
@pytest.mark.parametrize("players", [2, 3, 4])
def test_rollout_plan_rounds_up_to_whole_launches(steps, players):
    r = bench.REFILL_EVERY[players]
    p = bench.step_plan("rollout", steps, 5, r, rollout_k=64)
    assert p["per"] == 64
    assert p["K"] >= steps and p["K"] % p["unit"] == 0
    assert p["K"] % 64 == 0 and (p["K"] // 64) % 2 == 0  # action buffers alternate per launch
    assert p["K"] % r == 0                                # whole refill periods
    assert p["launches"] * p["per"] == p["K"]
    assert p["W"] >= 64 + r or p["W"] >= p["unit"]        # one full launch and a refill cycle
    assert p["W"] >= 64 and p["W"] % p["unit"] == 0
    assert p["G"] == 0                                    # rollout mode is timed eagerly
    assert p["launches"] >= bench.MIN_TIMED_LAUNCHES      # never a two-launch timed region
    # smallest whole-unit cover of max(steps, MIN_TIMED_LAUNCHES launches)
    assert p["K"] - max(steps, bench.MIN_TIMED_LAUNCHES * 64) < p["unit"]


@pytest.mark.parametrize("steps", [1, 20, 100, 1024])
def test_step_plan_graph_divides_timed_steps(steps):
    p = bench.step_plan("step", steps, 5, 64, graph_steps=128)
    assert p["per"] == 1 and p["unit"] == 64
    assert p["K"] >= steps and p["K"] % 64 == 0
    assert p["G"] > 0 and p["G"] % p["unit"] == 0 and p["K"] % p["G"] == 0
    assert p["G"] <= max(128, p["unit"])
    assert p["W"] >= 64


def test_driver_command_values():
    # step_plan at the driver's --steps 20 --warmup 5: eight 128-step launches timed (bench.ROLLOUT_K = 128,
    # ppo_splendor.py --num-steps; >= 16 ms of GPU time, VERDICT r02 "Next round" 1), two warmed up
    assert bench.ROLLOUT_K == 128 and bench.MIN_TIMED_LAUNCHES == 8
    p = bench.step_plan("rollout", 20, 5, 64)
    assert (p["K"], p["W"], p["launches"]) == (1024, 256, 8)
    p64 = bench.step_plan("rollout", 20, 5, 64, rollout_k=64)
    assert (p64["K"], p64["W"], p64["launches"]) == (512, 128, 8)
    s = bench.step_plan("step", 20, 5, 64)  # at least four replays of a full 128-step graph
    assert (s["K"], s["W"], s["G"]) == (512, 64, 128) and s["K"] // s["G"] == bench.MIN_TIMED_REPLAYS


def test_eager_step_plan_and_disabled_refill():
    p = bench.step_plan("step", 20, 0, 0, graph_steps=0)
    assert p["G"] == 0 and p["unit"] == 2 and p["K"] == 20 and p["launches"] == 20
    q = bench.step_plan("rollout", 200, 0, 0, rollout_k=16)
    assert q["unit"] == 32 and q["K"] == 224 and q["launches"] == 14
    q1 = bench.step_plan("rollout", 1, 0, 0, rollout_k=16, min_launches=1)
    assert q1["K"] == 32 and q1["launches"] == 2


@pytest.mark.parametrize("steps", [1, 20, 128, 300, 1024])
def test_headline_plan_times_exactly_the_requested_steps(steps):
    """The headline (headline_plan) times --steps env steps, whatever the value: whole launches and one
    shorter last launch in rollout mode, whole graphs and an eager tail in step mode."""
    p = bench.headline_plan("rollout", steps, 5, 64)
    assert p["K"] == steps and sum(p["sizes"]) == steps and p["launches"] == len(p["sizes"])
    assert all(s == 128 for s in p["sizes"][:-1]) and 1 <= p["sizes"][-1] <= 128
    assert p["G"] == 0 and p["W"] == 256  # warm-up: whole units, as step_plan's
    s = bench.headline_plan("step", steps, 5, 64)
    assert s["K"] == steps and s["replays"] * s["G"] + s["tail"] == steps
    assert s["G"] % 64 == 0 and s["G"] <= 128 and (s["G"] > 0) == (steps >= 64) and s["tail"] < max(s["G"], 64)
    assert s["W"] == 64
    assert bench.headline_plan("step", steps, 5, 64, graph_steps=0)["G"] == 0


def test_dump_sample_is_fixed_sorted_and_bounded():
    import numpy as np
    assert np.array_equal(bench.dump_sample(1000), np.arange(1000))
    a, b = bench.dump_sample(65536), bench.dump_sample(65536)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_TABLES and len(np.unique(a)) == len(a)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 65536
    # the rows --dump-outputs writes per table, as float32: two observation rows, the mask, eight scalars
    assert bench.DUMP_TABLES * 4 * (2 * 297 + 45 + 8) + bench.DUMP_TABLES * 8 <= 64 << 20


def test_algorithmic_bytes_constants():
    # SURVEY.md §8d (1370 / 1446) + the 16 B of the legal-mask cache (round 6)
    assert bench.STEP_ALGO_BYTES[2] == 1370 + 16 and bench.STEP_ALGO_BYTES[4] == 1446 + 16
    assert bench.OUT_BYTES == 1240


def test_step_shape_names_follow_the_library_rule():
    """bench.py names spl_step's kernel as the library picks it (spl_engine.hip spl_step: three waves up to
    two 64-table workgroups per CU, two above; a forced --step-tail wins)."""
    assert bench.step_shape("auto", 65536, cus=256) == 0 and bench.step_shape("auto", 32768, cus=256) == 1
    assert bench.step_shape("auto", 16384, cus=256) == 1 and bench.step_shape("2", 65536, cus=256) == 2
    assert bench.step_shape("auto", 49152, cus=256) == 1 and bench.step_shape("auto", 49153, cus=256) == 0
    assert [bench.STEP_SHAPE_SUFFIX[i] for i in range(3)] == ["ws", "wst", "wso"]
