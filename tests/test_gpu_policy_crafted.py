"""The three policy precisions (spl_policy.hip: bf16; spl_policy32.hip: the exact three-bf16-plane format and the
two-fp16-plane format, ring and narrow kernels) on the crafted networks of crafted_nets.py, against numpy float64.

Tolerances, and where each comes from (test_policy_crafted_host.py shows that each can fail):
  * tanh probes, exact format: 4 ulp of the float32 nearest float64 tanh on the layer-2 probe (tanh_acc with 1-ulp
    v_exp_f32 and v_rcp_f32 is at most 3.2 ulp, rounded up), 9 ulp on the layer-1 probe (two applications and one
    rounding; tanh's relative condition number is at most 1);
  * tanh probes, fp16-plane format: test_gpu_policy.fp32_close, 1e-5 x (|ref| + 1); bf16: 2e-2 against bf16_ref of
    the crafted module and 0.15 against float64, as test_greedy_logits_match_torch_bf16;
  * range networks and observation sweeps (fp32 forms): fp32_close on logits and value; the "out" network's
    layer-3 rows |got - ref| <= 64 x 2^-24 x (sum_k |w_k h_k| + |b|) per output (test_gpu_ppo_net.py's factor, per
    row because the rows are 2^60 apart); compact rows give the int32 rows' bytes;
  * logit tables: log-prob and entropy within atol = rtol = 1e-5 (bf16 1e-4) of a float64 log-softmax over the
    allowed set (test_full_image_serves_greedy_and_sample's); frequencies within 4 standard errors + 1e-6
    (test_sample_frequencies_match_softmax's); greedy equals the first maximum on every row, no near-tie exclusion.
The grouped launch (the only way into the narrow kernels) must give the plain launch's bits, as
test_gpu_opponent_pool.py demands of random networks."""
import ctypes

import numpy as np
import pytest

import crafted_nets as cn
from crafted_nets import NA
from test_gpu_policy import bf16_ref, fp32_close

pytestmark = pytest.mark.gpu
FP32_FORMS = ["fp32", "fp32_f16x2"]
ALL = FP32_FORMS + ["bf16"]
DEV = "cuda"


def batch(precision):
    """145 for the fp32 forms: a full 128-table workgroup and a ragged rest; 289 for bf16: 256 and a ragged rest."""
    return 289 if precision == "bf16" else 145


def dev(x, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def run(agent, precision, obs, mask=None, seed=3, ply=1):
    """One SAMPLE launch with logits: float64 logits [n, 45] and value [n], and the device tensors."""
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    n = len(obs)
    mask = np.ones((n, NA), dtype=np.int8) if mask is None else mask
    f = FusedActorCritic(agent.to(DEV), with_critic=True, precision=precision)
    action, logprob, entropy, value, logits = f.act(dev(obs), dev(mask), seed=seed, ply=ply, want_logits=True)
    torch.cuda.synchronize()
    return {"logits": logits.double().cpu().numpy(), "value": value.double().cpu().numpy()[:, 0], "f": f,
            "t": (action, logprob, entropy, value, logits)}


def tile_rows(n):
    rows = cn.real_rows(145)
    return np.ascontiguousarray(np.resize(rows, (n, rows.shape[1])))


# ---- tanh probes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ALL)
@pytest.mark.parametrize("layer", [2, 1])
@pytest.mark.parametrize("image", range(cn.PROBE_IMAGES))
def test_tanh_probes(precision, layer, image):
    """Logit j is the kernel's tanh of a chosen argument (twice, through the plane split, for layer 1), the value
    the critic's: every table gives the same 46 numbers, judged by the precision's tolerance."""
    import torch
    n = batch(precision)
    agent = cn.probe_agent(layer, image)
    out = run(agent, precision, tile_rows(n))
    arg, want = cn.probe_expected(layer, image)
    got = np.column_stack([out["logits"], out["value"]])
    assert (got == got[0]).all()  # every table, the ragged workgroup's too
    got = got[0]
    below = np.abs(arg) < float(cn.BRANCH)
    if precision == "fp32":
        u = cn.ulps(got, want)
        sites = {"ring below 0.625": u[:NA][below[:NA]], "ring from 0.625": u[:NA][~below[:NA]], "critic": u[NA:]}
        print(f"tanh_acc fp32 layer-{layer} probe image {image}: " + ", ".join(f"{k} {v.max():.3f} ulp" for k, v in sites.items() if len(v)))
        assert (u <= cn.PROBE_ULPS[layer]).all(), (arg[u > cn.PROBE_ULPS[layer]], u.max())
        assert (np.sign(got) == np.sign(want)).all()
        if layer == 2:
            assert (got[np.abs(arg) >= cn.SATURATED] == np.sign(arg[np.abs(arg) >= cn.SATURATED])).all()
    elif precision == "fp32_f16x2":
        err = np.abs(got - want)
        print(f"tanh_fold fp32_f16x2 layer-{layer} probe image {image}: max |error| logits {err[:NA].max():.3e} value {err[NA]:.3e}")
        assert (err <= 1e-5 * (np.abs(want) + 1)).all(), err.max()
    else:
        x = dev(tile_rows(1))
        with torch.no_grad():
            m = agent.to(DEV)
            ref16 = np.concatenate([bf16_ref(m.actor, x)[0].double().cpu().numpy(), bf16_ref(m.critic, x)[0].double().cpu().numpy()])
        print(f"tanh_fast bf16 layer-{layer} probe image {image}: against bf16_ref {np.abs(got - ref16).max():.3e}, against float64 "
              f"{np.abs(got - want).max():.3e}, value (fp32 tanh_fast, unrounded) {abs(got[NA] - want[NA]):.3e}")
        assert np.abs(got - ref16).max() <= 2e-2 and np.abs(got - want).max() <= 0.15


# ---- the grouped launch: ring and narrow kernels -------------------------------------------------------------
def grouped_sets():
    obs = cn.range_obs()
    return {"layer2_a": lambda: [cn.probe_agent(2, i) for i in (0, 1, 2)], "layer2_b": lambda: [cn.probe_agent(2, i) for i in (3, 4, 5)],
            "layer1_a": lambda: [cn.probe_agent(1, i) for i in (0, 1, 2)], "layer1_b": lambda: [cn.probe_agent(1, i) for i in (3, 4, 5)],
            "range": lambda: [cn.range_agent("hidden", obs), cn.range_agent("out", obs), cn.sweep_agent(cn.obs_sweep("fp32_f16x2")[0])]}


@pytest.mark.parametrize("precision", FP32_FORMS)
@pytest.mark.parametrize("which", list(grouped_sets()))
def test_grouped_launch_gives_the_plain_launchs_bits(precision, which):
    """Three crafted images, 165 tables each (a full 128-table workgroup on k_act32 and a 37-table tail on
    k_act32_narrow), one raw spl_policy_act_grouped call in SAMPLE mode with logits: every table's logits, action,
    log-prob and entropy are the bits of the plain launch of its image.  For the probes the narrow kernel's tanh
    is thereby the ring kernel's, already held to 4 / 9 ulp."""
    import torch
    from splendor_gym import _native
    from splendor_gym.fused_policy import FusedActorCritic, OpponentPool
    ms = [m.to(DEV) for m in grouped_sets()[which]()]
    pool = OpponentPool(ms[0], pool_size=2, precision=precision)
    for m in ms[1:]:
        pool.add_snapshot(m)
    slots = [0] + list(pool.pool)
    n = 3 * 165
    rows = cn.real_rows(n)
    if which == "range":
        rows[165:330] = np.resize(cn.range_obs(), (165, rows.shape[1]))
        rows[330:] = np.resize(cn.obs_sweep("fp32_f16x2")[0][0], (165, rows.shape[1]))
    member = np.repeat(np.arange(3), 165)
    perm = np.random.default_rng(5).permutation(n)  # the groups' tables interleaved
    rows, member = np.ascontiguousarray(rows[perm]), member[perm]
    obs, mask = dev(rows), dev(np.ones((n, NA), dtype=np.int8))
    g = dev(np.array(slots, dtype=np.int32)[member])
    act = torch.empty(n, dtype=torch.int32, device=DEV)
    lp, ent = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    lg = torch.empty(n, NA, device=DEV)
    scratch = torch.zeros(int(pool.lib.spl_policy_group_scratch_bytes(n, pool.n_images)), dtype=torch.uint8, device=DEV)
    a = _native.ActArgs(obs=obs.data_ptr(), mask=mask.data_ptr(), action=act.data_ptr(), logprob=lp.data_ptr(),
                        entropy=ent.data_ptr(), value=None, logits=lg.data_ptr(), seed=41, ply=3, ply_base=None,
                        table0=0, mode=_native.ACT_SAMPLE, image=pool._prec << 1)
    _native.check(pool.lib, pool.lib.spl_policy_act_grouped(pool.images.data_ptr(), pool.image_bytes, pool.n_images,
                                                            g.data_ptr(), scratch.data_ptr(), n, ctypes.byref(a),
                                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for i, m in enumerate(ms):
        f = FusedActorCritic(m, with_critic=False, precision=precision)
        wa, wl, we, _, wlg = f.act(obs, mask, seed=41, ply=3, want_logits=True)
        sel = dev(member == i)
        assert int(sel.sum()) == 165
        assert torch.equal(lg[sel].view(torch.int32), wlg[sel].view(torch.int32)), i
        assert torch.equal(act[sel], wa[sel]) and torch.equal(lp[sel], wl[sel]) and torch.equal(ent[sel], we[sel]), i


# ---- range networks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", FP32_FORMS)
@pytest.mark.parametrize("kind", ["hidden", "out"])
def test_range_networks(precision, kind):
    """Rows of every layer scaled by powers of two, outliers and all-zero rows.  [hidden-fp32_f16x2] is the case
    that found tanh_fold's cancellation near 0: with the exp2 form alone the units of the rows scaled by 2^-12
    (~1e-4) were off by 1.2e-7 each, and their consumer columns, scaled by 2^12 (~240), put 5.6e-5 on a logit,
    5.14 x the bound (test_policy_crafted_host.py::test_hidden_range_tolerance_rejects_a_tanh_that_cancels_near_zero
    reproduces 4.8e-5 on the CPU).  tanh_fold now switches to a cubic below 2^-4."""
    obs = cn.range_obs()
    agent = cn.range_agent(kind, obs)
    r = cn.forward64(cn.params_of(agent), obs)
    out = run(agent, precision, obs)
    got = np.column_stack([out["logits"], out["value"]])
    want = np.column_stack([r["actor"]["y"], r["critic"]["y"]])
    err = np.abs(got - want)
    if kind == "hidden":
        ratio = err / (1e-5 * (np.abs(want) + 1))
        print(f"range hidden {precision}: worst error / fp32_close bound {ratio.max():.3f} (max |error| {err.max():.3e})")
        assert fp32_close(dev(got), dev(want)), err.max()
        assert (ratio <= 1).all()
    else:
        bound = cn.ROW_ULPS * np.column_stack([r["actor"]["mag"], r["critic"]["mag"]])
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
        worst = np.unravel_index(ratio.argmax(), ratio.shape)
        print(f"range out {precision}: worst error / row bound {ratio.max():.3f} at output {worst[1]}; dominated rows "
              f"{ratio[:, list(cn.L3_OUTLIERS)].max(axis=0).round(3).tolist()}")
        assert (got[:, list(cn.L3_ZERO)] == 0).all()  # an all-zero row with a zero bias gives exactly 0
        assert (err <= bound).all(), (ratio.max(), worst)


# ---- observation sweeps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,fmt", [("fp32", "fp32"), ("fp32", "fp32_f16x2"), ("fp32_f16x2", "fp32_f16x2")])
@pytest.mark.parametrize("launch", range(cn.SWEEP_LAUNCHES))
def test_observation_sweeps(precision, fmt, launch):
    """One value beyond the bf16 plane (the exact format) or beyond 1024 (both) in every column: in one table of a
    wave, in all 16, in the ragged workgroup, with both signs."""
    obs, _ = cn.obs_sweep(fmt)
    agent = cn.sweep_agent(obs)
    want = np.column_stack(cn.outputs64(agent, obs[launch]))
    out = run(agent, precision, obs[launch])
    got = np.column_stack([out["logits"], out["value"]])
    ratio = np.abs(got - want) / (1e-5 * (np.abs(want) + 1))
    print(f"observation sweep {fmt} values on {precision}, launch {launch}: worst error / fp32_close bound {ratio.max():.3f}")
    assert fp32_close(dev(got), dev(want)) and (ratio <= 1).all(), ratio.max()


@pytest.mark.parametrize("precision", FP32_FORMS)
def test_compact_rows(precision):
    """All bytes 0, bytes 0..296 all 255, byte 297 = 0, 1 and the format's largest: the compact rows give the bytes
    of the int32 rows of the same values, and both are within fp32_close of float64."""
    import torch
    rows = cn.compact_rows(precision)
    x = cn.expand(rows)
    agent = cn.sweep_agent(x)
    mask = np.ones((len(rows), NA), dtype=np.int8)
    mask[::3, ::2] = 0
    a = run(agent, precision, x, mask)
    b = run(agent, precision, rows, mask)
    for ta, tb in zip(a["t"], b["t"]):
        assert torch.equal(ta, tb)
    want = np.column_stack(cn.outputs64(agent, x))
    got = np.column_stack([a["logits"], a["value"]])
    ratio = np.abs(got - want) / (1e-5 * (np.abs(want) + 1))
    print(f"compact rows {precision}: worst error / fp32_close bound {ratio.max():.3f}")
    assert (ratio <= 1).all(), ratio.max()


# ---- logit tables ---------------------------------------------------------------------------------------
def mask_rows(n):
    ms = cn.masks()
    names = list(ms)
    return [names[i % len(names)] for i in range(n)], np.stack([ms[names[i % len(names)]] for i in range(n)])


@pytest.mark.parametrize("precision", ALL)
@pytest.mark.parametrize("name", list(cn.logit_tables()))
def test_logit_tables(precision, name):
    """Every table's logits are exactly the chosen row; rows cycle through the seven masks.  SAMPLE: the action is
    allowed, log-prob and entropy are the float64 log-softmax's over the allowed set, the entropy is finite and not
    below -1e-6, one legal action gives that action with log-prob 0 and entropy 0 exactly.  GREEDY: the first maximum
    of the masked row, on every row."""
    import torch
    row = cn.logit_tables()[name]
    n = batch(precision)
    names, mask = mask_rows(n)
    agent = cn.logit_agent(row)
    out = run(agent, precision, tile_rows(n), mask, seed=17, ply=2)
    assert (out["logits"] == row.astype(np.float64)).all()
    action, logprob, entropy = (t.double().cpu().numpy() for t in out["t"][:3])
    action = action.astype(np.int64)
    tol = 1e-4 if precision == "bf16" else 1e-5
    worst = [0.0, 0.0]
    for i in range(n):
        allow = cn.allowed_set(mask[i])
        logp, ent = cn.log_softmax64(row, allow)
        assert allow[action[i]], (i, names[i])
        e_lp, e_en = abs(logprob[i] - logp[action[i]]), abs(entropy[i] - ent)
        worst = [max(worst[0], e_lp / (tol + tol * abs(logp[action[i]]))), max(worst[1], e_en / (tol + tol * abs(ent)))]
        assert e_lp <= tol + tol * abs(logp[action[i]]) and e_en <= tol + tol * abs(ent), (i, names[i], logprob[i], entropy[i])
        assert np.isfinite(entropy[i]) and entropy[i] >= -1e-6
        if names[i].startswith("only_"):
            assert action[i] == int(names[i][5:]) and logprob[i] == 0 and entropy[i] == 0, (i, names[i])
    print(f"logit table {name} {precision}: worst log-prob error / bound {worst[0]:.3f}, entropy {worst[1]:.3f}")
    greedy = out["f"].greedy(dev(tile_rows(n)), dev(mask)).cpu().numpy()
    want = np.array([cn.first_max(row, mask[i]) for i in range(n)])
    assert np.array_equal(greedy, want), (name, np.flatnonzero(greedy != want)[:5])


@pytest.mark.parametrize("precision", ALL)
def test_no_legal_action_samples_the_raw_logits(precision):
    """A row without a legal action samples from all 45 logits: with action 7 ninety above the rest it is action 7,
    with log-prob 0 to 1e-5; greedy gives 0."""
    row = cn.logit_tables()["peak90_group0"].copy()
    row[cn.PEAKS[0]] = row[0]
    row[7] = np.float32(np.delete(row, 7).max() + 90)
    n = batch(precision)
    mask = np.zeros((n, NA), dtype=np.int8)
    out = run(cn.logit_agent(row), precision, tile_rows(n), mask, seed=23, ply=5)
    assert (out["t"][0] == 7).all() and (out["t"][1].abs() <= 1e-5).all()
    assert (out["f"].greedy(dev(tile_rows(n)), dev(mask)) == 0).all()


@pytest.mark.parametrize("precision", ALL)
@pytest.mark.parametrize("table", list(cn.frequency_tables()))
@pytest.mark.parametrize("mname", cn.FREQUENCY_MASKS)
def test_sampling_frequencies(precision, table, mname):
    """65 536 tables of one row under one mask: the frequencies are the float64 softmax's to 4 standard errors +
    1e-6; nothing outside the mask is drawn.  The draw is keyed by (seed; table, ply), so the outcome is fixed."""
    from splendor_gym.fused_policy import FusedActorCritic
    n = 65536
    row, mask = cn.frequency_tables()[table], cn.masks()[mname]
    agent = cn.logit_agent(row).to(DEV)
    obs = dev(tile_rows(1)).repeat(n, 1).contiguous()
    k = dev(mask).view(1, NA).repeat(n, 1).contiguous()
    f = FusedActorCritic(agent, with_critic=True, precision=precision)
    act = f.act(obs, k, seed=99, ply=0)[0].cpu().numpy()
    p = np.exp(cn.log_softmax64(row, cn.allowed_set(mask))[0])
    freq = np.bincount(act, minlength=NA) / n
    se = np.sqrt(p * (1 - p) / n) + 1e-9
    ratio = np.abs(freq - p) / (4 * se + 1e-6)
    print(f"frequencies {table} {mname} {precision}: worst deviation / bound {ratio.max():.3f}")
    assert freq[mask == 0].sum() == 0
    assert (ratio <= 1).all(), (freq, p)
