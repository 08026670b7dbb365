"""The crafted networks of crafted_nets.py without a GPU: each builder does what it says (through the float64
oracle), a float32 emulation of tanh_acc against float64 tanh, and the sensitivity of every comparison of
test_gpu_policy_crafted.py / test_gpu_ppo_net_crafted.py: a deliberately wrong float64 oracle, evaluated on the
very inputs the GPU tests run, must leave the tolerance of the comparison it is aimed at in every case that
comparison parametrises.  A tolerance a wrong kernel could not fail would check nothing."""
import numpy as np
import pytest

import crafted_nets as cn
from crafted_nets import H, IN, NA, NETS, params_of

FP32_FORMS = ("fp32", "fp32_f16x2")


# ---- construction ---------------------------------------------------------------------------------------
def test_sweep_holds_every_chosen_argument_with_both_signs():
    s = cn.sweep()
    assert s.dtype == np.float32 and s.shape == (H,)
    for m in cn.special_magnitudes():
        assert (s == m).any() and (s == -m).any(), m
    t1 = cn.tanh_one()
    assert np.float32(np.tanh(np.float64(t1))) == 1 and np.float32(np.tanh(np.float64(cn._next(t1, -1)))) < 1
    assert abs(float(t1) - 9.01) < 0.01
    small, large = np.abs(s) < cn.BRANCH, np.abs(s) >= cn.BRANCH
    assert small.sum() >= 64 and large.sum() >= 64  # both branches, many times
    assert (np.abs(s) >= cn.SATURATED).sum() >= 14


@pytest.mark.parametrize("layer", [1, 2])
def test_probe_outputs_are_tanh_of_the_sweep_exactly(layer):
    """Through the float64 oracle a probe's 45 logits and its value EQUAL np.tanh (once or twice) of the chosen
    arguments: no other operation rounds.  The six images read every hidden unit; the critic's read six tiles."""
    read = set()
    for image in range(cn.PROBE_IMAGES):
        agent = cn.probe_agent(layer, image)
        logits, value = cn.outputs64(agent, cn.real_rows(3))
        arg, want = cn.probe_expected(layer, image)
        a, c = cn.probe_biases(image)
        assert np.array_equal(arg[:NA], a[cn.probe_units(image)].astype(np.float64)) and arg[NA] == np.float64(c[cn.CRITIC_UNITS[image]])
        for r in range(3):
            assert np.array_equal(logits[r], want[:NA]) and value[r] == want[NA]
        assert np.array_equal(want, np.tanh(arg) if layer == 2 else np.tanh(np.tanh(arg)))
        read |= set(cn.probe_units(image).tolist())
        # the float32 parameters hold the sweep exactly
        got = params_of(agent)["actor"][3 if layer == 2 else 1]
        assert np.array_equal(got, a.astype(np.float64))
    assert read == set(range(H))
    assert len({u // 16 for u in cn.CRITIC_UNITS}) == 6 and {(u % 16) % 4 for u in cn.CRITIC_UNITS} == {0, 1, 2, 3}
    assert (np.abs(cn.critic_values()) < cn.BRANCH).sum() == 3


@pytest.mark.parametrize("kind", ["hidden", "out"])
def test_range_networks_stay_unsaturated_and_inside_the_packs_clamp(kind):
    obs = cn.range_obs()
    agent = cn.range_agent(kind, obs)
    p = params_of(agent)
    r = cn.forward64(p, obs)
    for net in NETS:
        assert max(np.abs(r[net]["z1"]).max(), np.abs(r[net]["z2"]).max()) < 3.0, net
        for w in p[net][0::2]:
            top = np.abs(w).max(axis=1)
            assert ((top == 0) | ((top >= 2.0 ** -40) & (top <= 2.0 ** 40))).all()
    w1, b1, w2, b2, w3, b3 = p["actor"]
    if kind == "hidden":
        base = params_of(cn.new_agent(31))["actor"]
        assert not w1[list(cn.L1_ZERO)].any() and not w2[list(cn.L2_ZERO)].any()
        assert (r["actor"]["h1"][:, list(cn.L1_ZERO)] == 0).all() and (r["actor"]["h2"][:, list(cn.L2_ZERO)] == 0).all()
        for row, k, e in cn.L2_OUTLIERS:  # the outlier is the row's largest entry by far, on an input that is 0
            assert abs(w2[row, k]) == np.abs(w2[row]).max() > 2.0 ** (e - 4) * np.median(np.abs(w2[row])) and k in cn.L1_ZERO
        assert np.allclose(w1[3], 0.4 * base[0][3] * 2.0 ** -12, rtol=1e-6, atol=0) and w2[9, 3] == base[2][9, 3] * 2.0 ** 12
        spread = np.abs(w2[9][w2[9] != 0])
        assert spread.max() / spread.min() > 2.0 ** 12
    else:
        assert not w3[list(cn.L3_ZERO)].any() and not b3[list(cn.L3_ZERO)].any()
        assert (r["actor"]["y"][:, list(cn.L3_ZERO)] == 0).all()
        tops = np.abs(w3).max(axis=1)
        assert tops[tops > 0].max() / tops[tops > 0].min() > 2.0 ** 55
        for j in cn.L3_OUTLIERS:  # one product dominates the row on every table
            terms = np.abs(r["actor"]["h2"] * w3[j])
            assert (terms.max(axis=1) > 0.95 * (terms.sum(axis=1) + abs(b3[j]))).all(), j


@pytest.mark.parametrize("fmt", FP32_FORMS)
def test_observation_sweeps_cover_every_column_in_one_table_and_in_all(fmt):
    obs, col = cn.obs_sweep(fmt)
    limit = 256 if fmt == "fp32" else 1024
    big = np.abs(obs) >= limit
    assert np.abs(obs).max() < (2 ** 16 if fmt == "fp32" else 2048)
    one, every = np.zeros(IN, bool), np.zeros(IN, bool)
    for L in range(cn.SWEEP_LAUNCHES):
        for w0 in range(0, cn.SWEEP_N, 16):
            count = big[L, w0:w0 + 16].sum(axis=0)
            rows = min(16, cn.SWEEP_N - w0)
            one |= count == 1
            every |= (count == rows) & (rows == 16)
    assert one.all() and every.all()
    vals = obs[big].astype(np.float64)
    if fmt == "fp32":  # the bf16 plane does not hold them: the residual plane is needed for every one
        assert (cn.round_bits(vals, 8) != vals).all()
        assert {257, -257, 333, -333, 383, -383, 32769, -32769, 65407, -65407} == set(obs[big].tolist())
    else:
        assert set(obs[big].tolist()) == {1025, -1025, 2047, -2047}
        assert (vals.astype(np.float16).astype(np.float64) == vals).all()  # "exact in fp16"
    r = cn.forward64(params_of(cn.sweep_agent(obs)), obs.reshape(-1, IN))
    for net in NETS:
        assert max(np.abs(r[net]["z1"]).max(), np.abs(r[net]["z2"]).max()) < 3.0


@pytest.mark.parametrize("fmt", FP32_FORMS + ("ppo",))
def test_compact_rows(fmt):
    rows = cn.compact_rows(fmt)
    top = 7 if fmt == "fp32_f16x2" else 255
    assert rows.dtype == np.uint8 and rows.shape == (cn.SWEEP_N, 300) and not rows[0].any()
    assert (rows[1:4, :IN] == 255).all() and rows[1:4, 297].tolist() == [0, 1, top]
    assert set(rows[:, 297].tolist()) == {0, 1, top} and not rows[:, 298:].any()
    x = cn.expand(rows)
    assert x[3, 295] == 255 + 256 * top and np.array_equal(cn.compact(x), rows)
    assert set(rows[-3:, 297].tolist()) == {0, 1, top}  # in the ragged last wave too


def test_logit_agents_give_the_row_exactly():
    for name, row in list(cn.logit_tables().items())[::5]:
        logits, _ = cn.outputs64(cn.logit_agent(row), cn.real_rows(5))
        assert (logits == row.astype(np.float64)).all(), name
    t = cn.logit_tables()
    assert len(t) == 12 + 3 + 5
    for gap in (20, 90, 200):
        for g, k in enumerate(cn.PEAKS):
            row = t[f"peak{gap}_group{g}"]
            assert cn.GROUPS[g][0] <= k < cn.GROUPS[g][1] and row[k] - np.delete(row, k).max() == gap
    for name, members in cn.TIES.items():
        row = t[name]
        assert np.flatnonzero(row == row.max()).tolist() == sorted(members)
    assert len({next(g for g, (a, b) in enumerate(cn.GROUPS) if a <= k < b) for k in cn.TIES["tie_four"]}) == 4
    mild = cn.frequency_tables()["mild"]
    assert mild.max() - mild.min() <= 3


# ---- tanh_acc in numpy float32 ---------------------------------------------------------------------------
F = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def tanh_acc_emulated(x, exp_ulps=0, rcp_ulps=0):
    """spl_policy32.hip's tanh_acc (and spl_ppo_net_common.h's copy): the same coefficients in the same order;
    exp2 and the reciprocal correctly rounded, then moved by the given number of float32 steps."""
    x = np.asarray(x, dtype=np.float32)
    ax = np.abs(x)
    with np.errstate(over="ignore", invalid="ignore"):  # the unselected polynomial overflows on large arguments, as on the device
        z = ax * ax
        p = np.full_like(ax, F(-0.005718891508877277))
        for c in (0.02065306343138218, -0.053744640201330185, 0.13331513106822968, -0.3333328664302826):
            p = _fma(p, z, np.full_like(ax, F(c)))
        small = _fma(ax * z, p, ax)
        e = np.exp2((ax * F(2.8853900817779268)).astype(np.float64)).astype(np.float32)

    def step(v, n):
        for _ in range(abs(n)):
            v = np.nextafter(v, F(np.inf if n > 0 else -np.inf))
        return v

    e = step(e, exp_ulps)
    rcp = step((1.0 / (e + F(1.0)).astype(np.float64)).astype(np.float32), rcp_ulps)
    big = _fma(np.full_like(ax, F(-2.0)), rcp, np.full_like(ax, F(1.0)))
    return np.copysign(np.where(ax < F(0.625), small, big), x)


def tanh_grid():
    g = np.concatenate([np.abs(cn.sweep()), np.exp(np.linspace(np.log(2.0 ** -126), np.log(100.0), 200001)),
                        np.linspace(0.5, 1.0, 100001), np.linspace(0.0, 12.0, 100001)[1:]]).astype(np.float32)
    return np.unique(g[g >= F(2.0 ** -126)])


def test_tanh_acc_emulation_against_float64():
    """With correctly rounded exp2 and reciprocal: at most 1.7 ulp anywhere (1.63 measured, at x ~ 0.6315) and
    at most 0.9 ulp on the polynomial branch (0.80 measured); with each of the two moved one step in the worst
    direction at most 2.7 ulp (2.63).  These back the 4 ulp the GPU tests allow the kernels (the analytic worst
    case with 1-ulp v_exp_f32 and v_rcp_f32 is 3.2 ulp, at the 0.625 boundary)."""
    x = tanh_grid()
    want = np.tanh(x.astype(np.float64))
    err = cn.ulps(tanh_acc_emulated(x), want)
    poly = x < cn.BRANCH
    print(f"tanh_acc emulation: polynomial branch {err[poly].max():.3f} ulp, exp2 branch {err[~poly].max():.3f} ulp at x = "
          f"{x[~poly][err[~poly].argmax()]:.6f}, {len(x)} points")
    assert err[poly].max() <= 0.9 and err.max() <= 1.7
    worst = max(cn.ulps(tanh_acc_emulated(x, a, b), want)[~poly].max() for a in (-1, 1) for b in (-1, 1))
    print(f"tanh_acc emulation, exp2 and rcp each one step off: {worst:.3f} ulp")
    assert 1.7 < worst <= 2.7
    # odd, exact at 0, the identity where x^3 / 3 is below half a step of x
    assert tanh_acc_emulated(F(0.0)) == 0 and tanh_acc_emulated(F(2.0 ** -126)) == F(2.0 ** -126)
    assert np.array_equal(tanh_acc_emulated(-x), -tanh_acc_emulated(x))
    assert (tanh_acc_emulated(np.array([20.0, 44.0, 45.0, 88.0, 1e4, 3e38], dtype=np.float32)) == 1).all()


# ---- sensitivity ---------------------------------------------------------------------------------------
def tanh_exp_form32(x, factor=1.0):
    """1 - 2 / (exp2(2 log2(e) |x|) + 1) in float32 (tanh_fold / tanh_fast without tanh_acc's polynomial);
    factor: a wrong tanh factor."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        e = np.exp2((np.abs(x).astype(np.float32) * F(2.8853900817779268 * factor)).astype(np.float64)).astype(np.float32)
        y = F(1.0) - F(2.0) * (F(1.0) / (e + F(1.0))).astype(np.float32)
    return np.copysign(y.astype(np.float64), x)


@pytest.mark.parametrize("layer", [1, 2])
@pytest.mark.parametrize("image", range(cn.PROBE_IMAGES))
def test_probe_bounds_reject_a_wrong_tanh(layer, image):
    """Exact format, 4 / 9 ulp: tanh from the exp2 form alone (absolute error ~6e-8) leaves the bound on the
    near-zero probes of every image, value included.  fp16-plane format (fp32_close) and bf16 (2e-2): a tanh
    factor that is off by two leaves both on every image."""
    arg, want = cn.probe_expected(layer, image)
    apply = (lambda f, x: f(f(x))) if layer == 1 else (lambda f, x: f(x))
    near_zero = (np.abs(arg) < 1e-3) & (arg != 0)
    assert near_zero[:NA].sum() >= 5
    bad = cn.outside(cn.ulps(apply(tanh_exp_form32, arg), want), cn.PROBE_ULPS[layer])
    assert bad[:NA][near_zero[:NA]].all()
    if abs(arg[NA]) < 1e-3:
        assert bad[NA]
    # the critic's probe: every image's value is within the bound when right ...
    assert not cn.outside(cn.ulps(apply(lambda x: tanh_acc_emulated(x).astype(np.float64), arg), want), cn.PROBE_ULPS[layer]).any()
    doubled = apply(lambda x: np.tanh(2.0 * x), arg)
    assert cn.fp32_outside(doubled, want)[:NA].sum() >= 5 and (np.abs(doubled - want)[:NA] > 2e-2).sum() >= 3
    # ... and all six together see a wrong factor in the critic's unit
    crit = [cn.probe_expected(layer, i) for i in range(cn.PROBE_IMAGES)]
    assert sum(bool(cn.fp32_outside(apply(lambda x: np.tanh(2.0 * x), a[NA]), w[NA])) for a, w in crit) >= 3


@pytest.mark.parametrize("fmt", FP32_FORMS)
@pytest.mark.parametrize("launch", range(cn.SWEEP_LAUNCHES))
def test_sweep_tolerance_rejects_rounded_observations(fmt, launch):
    """Observations rounded to the bf16 plane (the residual plane dropped) for the exact format; for the fp16
    planes, whose own rounding of a value below 2048 is the identity, to one bit fewer (10 significant bits) and
    to the bf16 plane: fp32_close fails in every launch: on every all-table row, and on every single row
    by itself but those of 32 769, whose residual is a part in 32 769 of one weight's product.""" 
    obs, col = cn.obs_sweep(fmt)
    agent = cn.sweep_agent(obs)
    x = obs[launch].astype(np.float64)
    want = np.column_stack(cn.outputs64(agent, x))
    for bits in ((8,) if fmt == "fp32" else (10, 8)):
        got = np.column_stack(cn.outputs64(agent, cn.round_bits(x, bits)))
        bad = cn.fp32_outside(got, want).any(axis=1)
        single = col[launch] >= 0
        print(f"{fmt} launch {launch} rounded to {bits} bits: {bad[single].sum()} of {single.sum()} single rows and "
              f"{bad[~single].sum()} of {(~single).sum()} all-table rows leave fp32_close")
        weak = np.abs(x).max(axis=1) == 32769
        assert bad[~single].all() and bad[single & ~weak].all() and (single & ~weak)[128:].any()


@pytest.mark.parametrize("fmt", FP32_FORMS + ("ppo",))
def test_compact_tolerance_rejects_a_dropped_high_byte(fmt):
    rows = cn.compact_rows(fmt)
    x = cn.expand(rows)
    agent = cn.sweep_agent(x)
    want = np.column_stack(cn.outputs64(agent, x))
    low = rows.copy()
    low[:, 297] = 0
    bad = cn.fp32_outside(np.column_stack(cn.outputs64(agent, cn.expand(low))), want).any(axis=1)
    assert bad[rows[:, 297] == rows[:, 297].max()].all() and not bad[rows[:, 297] == 0].any()


def _with_weights(p, f, which=(0, 2, 4)):
    return {net: [f(a) if i in which else a for i, a in enumerate(p[net])] for net in NETS}


def test_row_bound_rejects_a_dropped_third_plane():
    """Layer 3's per-row bound 64 x 2^-24 x (sum |w h| + |b|): weights rounded to 16 significant bits (the third
    bf16 plane dropped) leave it on the dominated rows 0 and 2 of every table; to 11 bits below the row's exponent
    (the second fp16 plane dropped) on rows 2 and 3 of every table (there the row's other entries, 2^-20 and 2^-12 of the outlier, round to nothing)."""
    obs = cn.range_obs()
    p = params_of(cn.range_agent("out", obs))
    r = cn.forward64(p, obs)
    for f, rows_hit in ((lambda w: cn.round_bits(w, 16), [0, 2]), (lambda w: cn.round_row_relative(w, 11), [2, 3])):
        m = cn.forward64(_with_weights(p, f), obs)
        for net in NETS:
            bad = cn.outside(np.abs(m[net]["y"] - r[net]["y"]), cn.ROW_ULPS * r[net]["mag"])
            if net == "actor":
                assert bad[:, rows_hit].all()
                assert not bad[:, list(cn.L3_ZERO)].any()  # exact zeros stay exact zeros
    # and the right answer in float32 arithmetic is inside it (64 steps of the row's magnitude)
    p32 = {net: [a.astype(np.float32) for a in p[net]] for net in NETS}
    h2 = r["actor"]["h2"].astype(np.float32)
    y32 = (h2 @ p32["actor"][4].T + p32["actor"][5]).astype(np.float64)
    assert not cn.outside(np.abs(y32 - r["actor"]["y"]), cn.ROW_ULPS * r["actor"]["mag"]).any()


def test_hidden_range_tolerance_rejects_dropped_planes():
    """fp32_close on the "hidden" network: one fp16 plane (11 bits below the row's exponent) and one bf16 plane
    (8 significant bits) each leave it.  Two bf16 planes (16 bits) cannot: 2^-17 per weight, summed with random
    signs over a row, is ~2e-6 on a logit, which is why the third plane is judged by the row bound above."""
    obs = cn.range_obs()
    p = params_of(cn.range_agent("hidden", obs))
    want = np.column_stack(cn.outputs64(p, obs))
    for f in (lambda w: cn.round_row_relative(w, 11), lambda w: cn.round_bits(w, 8)):
        for which in ((0,), (2,), (4,)):  # each layer alone
            got = np.column_stack(cn.outputs64(_with_weights(p, f, which), obs))
            assert cn.fp32_outside(got, want).any(), which
    # the outlier rows alone are enough for the fp16 plane
    w2 = p["actor"][2]
    only = w2.copy()
    rows = [r for r, _, _ in cn.L2_OUTLIERS]
    only[rows] = cn.round_row_relative(w2[rows], 11)
    q = {"actor": p["actor"][:2] + [only] + p["actor"][3:], "critic": p["critic"]}
    assert cn.fp32_outside(cn.outputs64(q, obs)[0], want[:, :NA]).any()


def tanh_fold_emulated(x, exp_ulps=0, rcp_ulps=0):
    """spl_policy32.hip's tanh_fold at S = 0 and a row factor of 1 (both are powers of two, so they move no
    rounding): t - t^3 / 3 from a = 2 log2(e) |x| below |x| = 2^-4, the exp2 form from there up; exp2 and the
    reciprocal correctly rounded, then moved by the given number of float32 steps."""
    x = np.asarray(x, dtype=np.float64)
    k = 2.8853900817779268
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.abs(x).astype(np.float32) * F(k)
        small = a * _fma(a * a, np.full_like(a, F(-1.0 / (3.0 * k * k * k))), np.full_like(a, F(1.0 / k)))
        e = np.exp2(a.astype(np.float64)).astype(np.float32)
        for _ in range(abs(exp_ulps)):
            e = np.nextafter(e, F(np.inf if exp_ulps > 0 else -np.inf))
        rcp = (1.0 / (e + F(1.0)).astype(np.float64)).astype(np.float32)
        for _ in range(abs(rcp_ulps)):
            rcp = np.nextafter(rcp, F(np.inf if rcp_ulps > 0 else -np.inf))
        big = _fma(np.full_like(a, F(-2.0)), rcp, np.full_like(a, F(1.0)))
    return np.copysign(np.where(a < F(0.0625 * k), small, big).astype(np.float64), x)


def test_tanh_fold_emulation_against_float64():
    """tanh_fold keeps the exp2 form's absolute error and, with its cubic below 2^-4, bounds the relative one.
    Absolute, exp2 and rcp each up to a step off: 1.5 steps of e near 1 (1.5 x 2^-23 x 2 / 4 = 8.9e-8), the
    rounding of e + 1 (2^-23 x 2 / 4 = 6.0e-8), 1.5 steps of the reciprocal (1.5 x 2^-25 x 2 = 8.9e-8) and the
    final rounding (3.0e-8): 2.7e-7.  Relative: 2 t^4 / 15 = 2.1e-6 of truncation under the switch,
    2.7e-7 / tanh(2^-4) = 4.4e-6 above it.  The exp2 form alone is 6e-8 / |x| off: 100 % at 1e-8."""
    x = tanh_grid()
    want = np.tanh(x.astype(np.float64))
    worst_abs = worst_rel = 0.0
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            err = np.abs(tanh_fold_emulated(x, a, b) - want)
            worst_abs, worst_rel = max(worst_abs, err.max()), max(worst_rel, (err / want).max())
    print(f"tanh_fold emulation, exp2 and rcp up to one step off: max |error| {worst_abs:.3e}, max relative error {worst_rel:.3e}")
    assert worst_abs <= 2.7e-7 and worst_rel <= 4.4e-6
    assert tanh_fold_emulated(0.0) == 0 and np.array_equal(tanh_fold_emulated(-x), -tanh_fold_emulated(x))
    assert (np.abs(tanh_exp_form32(x) - want) / want).max() > 0.5


def test_hidden_range_tolerance_rejects_a_tanh_that_cancels_near_zero():
    """fp32_close on the "hidden" range network: float64 with tanh as float32 1 - 2 / (exp2 + 1) on the eight
    down-scaled units alone, exact everywhere else, leaves it (4.8e-5: ~6e-8 on a unit of ~1e-4, times the 2^12 of
    its consumer column; the fp16-plane kernel did exactly this, 5.6e-5 on the MI355X, before tanh_fold got its
    cubic).  With tanh_fold's emulation on EVERY unit the network stays inside, exp2 and rcp a step off included."""
    obs = cn.range_obs()
    p = params_of(cn.range_agent("hidden", obs))
    want = np.column_stack(cn.outputs64(p, obs))
    calls = [0]

    def tanh(z):
        calls[0] += 1
        y = np.tanh(z)
        units = list(cn.L1_DOWN if calls[0] % 2 == 1 else cn.L2_DOWN)
        y[:, units] = tanh_exp_form32(z[:, units])
        return y

    err = np.abs(np.column_stack(cn.outputs64(p, obs, tanh=tanh)) - want)
    print(f"float32 exp-form tanh on the down-scaled units alone: max |error| {err.max():.3e}, "
          f"{(err / (1e-5 * (np.abs(want) + 1))).max():.2f} x the fp32_close bound")
    assert 3e-5 < err.max() < 1e-4 and cn.fp32_outside(np.column_stack(cn.outputs64(p, obs, tanh=tanh)), want).any()
    for a, b in ((0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)):
        got = np.column_stack(cn.outputs64(p, obs, tanh=lambda z: tanh_fold_emulated(z, a, b)))
        ratio = (np.abs(got - want) / (1e-5 * (np.abs(want) + 1))).max()
        print(f"tanh_fold emulation on every unit, exp2 {a:+d} rcp {b:+d} steps: {ratio:.3f} x the fp32_close bound")
        assert ratio <= 1


@pytest.mark.parametrize("name", ["equal_plus_1e4", "equal_minus_1e4"])
def test_softmax_tolerance_rejects_a_softmax_without_the_maximum(name):
    row = cn.logit_tables()[name]
    for mname, mask in cn.masks().items():
        allow = cn.allowed_set(mask)
        logp, ent = cn.log_softmax64(row, allow)
        bad_logp, bad_ent = cn.log_softmax64(row, allow, subtract_max=False, dtype=np.float32)
        k = int(np.flatnonzero(allow)[0])
        assert cn.outside(abs(bad_logp[k] - logp[k]), 1e-5 + 1e-5 * abs(logp[k])), mname
        assert cn.outside(abs(bad_ent - ent), 1e-5 + 1e-5 * abs(ent)), mname
        assert np.isclose(ent, np.log(allow.sum())) and np.isclose(logp[k], -np.log(allow.sum()))


@pytest.mark.parametrize("table", ["equal", "mild"])
@pytest.mark.parametrize("mname", cn.FREQUENCY_MASKS)
def test_frequency_tolerance_rejects_a_wrong_carry(table, mname):
    """4 standard errors + 1e-6 at 65 536 draws: a scan whose lane group g starts from 0 instead of the groups
    before it leaves it for every g that has allowed actions before it; under the last-group mask, where every
    carry is 0, a carry that counts disallowed actions does."""
    n = 65536
    row, mask = cn.frequency_tables()[table], cn.masks()[mname]
    allow = cn.allowed_set(mask)
    p = np.exp(cn.log_softmax64(row, allow)[0])
    se = np.sqrt(p * (1 - p) / n) + 1e-9
    assert np.abs(cn.scan_frequencies(row, mask) - p).max() < 1e-5  # the scan without a fault is the softmax
    if mname == "last_group":
        assert cn.outside(np.abs(cn.scan_frequencies(row, mask, ignore_mask_in_carry=True) - p), 4 * se + 1e-6).any()
        return
    for g in (1, 2, 3):
        assert cn.outside(np.abs(cn.scan_frequencies(row, mask, drop_carry=g) - p), 4 * se + 1e-6).any(), g


@pytest.mark.parametrize("name", list(cn.TIES))
def test_greedy_rule_rejects_the_last_maximum(name):
    row = cn.logit_tables()[name]
    members = cn.TIES[name]
    assert cn.first_max(row, cn.masks()["all"]) == min(members) != cn.first_max(row, cn.masks()["all"], last=True) == max(members)
    differ = [m for m, mask in cn.masks().items() if cn.first_max(row, mask) != cn.first_max(row, mask, last=True)]
    assert "all" in differ
    assert cn.first_max(row, cn.masks()["none"]) == 0
