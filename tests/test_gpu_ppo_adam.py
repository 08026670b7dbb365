"""The PPO optimiser step on the device (spl_ppo_adam, splendor_gym.ppo.DeviceAdam) against the float64
oracle of test_ppo_adam_host.py: segment sizes around the chunk, unaligned segments, determinism, the
target-KL gate and its latches, non-finite gradients, a captured step that follows set_lr, checkpoints in
torch's format, and ppo_update / ppo_device with the optimiser on the device.

Tolerances follow test_gpu_ppo_loss.py's rule.  The kernel and torch's float32 clip_grad_norm_ + Adam
evaluate one formula and differ in summation order and rounding, so the kernel may be as far from the
float64 oracle as max(4 x torch's float32 error on the same inputs, 64 x 2^-24 x scale): for a parameter
scale = max|p| + steps x lr, for the norm the norm itself.  Every comparison prints both errors first
(DESIGN.md has the table measured on an MI355X)."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_ppo_loss import DEV, allowed, collected  # noqa: F401  (collected: a module fixture)
from test_ppo_adam_host import KL_EPOCHS, STATS, TARGET_KL, adam_state, gate_sequence, make_problem, run_oracle

pytestmark = pytest.mark.gpu

LR, EPS, MAX_NORM = 2.5e-4, 1e-5, 0.5
STEPS = 5  # gradient scales 3, 1e-3, 0.05, 10, 1e-6: norms on both sides of MAX_NORM
AGENT_SHAPES = ((256, 297), (256,), (256, 256), (256,), (1, 256), (1,), (256, 297), (256,), (256, 256), (256,), (45, 256), (45,))


def chunk():
    from splendor_gym import _native
    return _native.PPO_ADAM_CHUNK


def on_device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays]


def give(params, grads):
    for p, g in zip(params, grads):
        p.grad = g


def bits(tensors):
    import torch
    return [x.detach().contiguous().view(torch.int32).clone() for x in tensors]


def run_device(params, grads, **kw):
    """DeviceAdam from zero moments over all steps; the state after each call."""
    from splendor_gym.ppo import DeviceAdam
    p = on_device(params)
    opt = DeviceAdam(p, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, **kw)
    states = []
    for g in grads:
        give(p, on_device(g))
        opt.step()
        assert all(x.grad is None for x in p)  # taken
        states.append(opt.read_state())
    return p, opt, states


def run_torch(params, grads):
    """clip_grad_norm_ + torch.optim.Adam in float32 on the GPU; the norm of each call."""
    import torch
    p = [torch.nn.Parameter(x) for x in on_device(params)]
    opt = torch.optim.Adam(p, lr=LR, eps=EPS)
    norms = []
    for g in grads:
        give(p, on_device(g))
        norms.append(float(torch.nn.utils.clip_grad_norm_(p, MAX_NORM)))
        opt.step()
    return p, opt, norms


def compare(label, got, ref, want, steps):
    """The tolerance rule on every parameter tensor; prints first."""
    worst = (0.0, 0.0, 0.0)
    for i, (a, b, w) in enumerate(zip(got, ref, want)):
        a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
        e_k, e_t, scale = float(np.abs(a - w).max()), float(np.abs(b - w).max()), float(np.abs(w).max()) + steps * LR
        worst = max(worst, (e_k, e_t, scale))
        assert e_k <= allowed(e_t, scale), (label, i, e_k, e_t, scale)
    print(f"{label} parameters: e_kernel {worst[0]:.3e} e_torch {worst[1]:.3e} scale {worst[2]:.3e}")


def compare_norms(label, states, norms, calls):
    worst = (0.0, 0.0, 0.0)
    for st, n_t, (n_o, coef, active) in zip(states, norms, calls):
        e_k, e_t = abs(st["grad_norm"] - n_o), abs(n_t - n_o)
        worst = max(worst, (e_k / n_o, e_t / n_o, n_o))
        assert e_k <= allowed(e_t, n_o), (label, e_k, e_t, n_o)
        assert st["active"] == active == 1
        assert abs(st["clip_coef"] - coef) <= 2.0 ** -22 * coef and (st["clip_coef"] == 1.0) == (coef == 1.0)
        assert st["clip_coef"] == float(np.float32(st["clip_coef"]))  # what the elements saw
    print(f"{label} norm (relative): e_kernel {worst[0]:.3e} e_torch {worst[1]:.3e}")


def shape_cases():
    C = chunk()
    mixed = (1, 3, 4, 5, 7, C - 1, C, C + 1, 2 * C + 3, 64, 2, 257, 1023, 8, 6, 4097)
    cases = [(f"one[{n}]", ((n,),)) for n in (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)]
    cases.append(("sixteen", tuple((n,) for n in mixed)))
    cases.append(("agent", AGENT_SHAPES))
    # more chunks than partial sums: the workgroups take a second chunk each
    cases.append(("wrap", ((513 * C + 5,), (3,))))
    return cases


@pytest.mark.parametrize("label,shapes", shape_cases(), ids=[c[0] for c in shape_cases()])
def test_shapes_against_the_oracle(label, shapes):
    params, grads = make_problem(shapes, 11, STEPS)
    state = adam_state(lr=LR, eps=EPS, max_norm=MAX_NORM)
    want, want_m, want_v, calls = run_oracle(params, grads, state)
    coefs = [c[1] for c in calls]
    assert min(coefs) < 1.0 and max(coefs) == 1.0  # clipped and unclipped calls both occur
    p, opt, states = run_device(params, grads)
    ref, ref_opt, norms = run_torch(params, grads)
    compare(label, p, ref, want, STEPS)
    compare_norms(label, states, norms, calls)
    # the moments: the same rule with their own magnitude as the scale
    sd = ref_opt.state_dict()["state"]
    for name, arena, oracle in (("exp_avg", opt._exp_avg, want_m), ("exp_avg_sq", opt._exp_avg_sq, want_v)):
        for i, (a, w) in enumerate(zip(opt._moments(arena), oracle)):
            e_k = float(np.abs(a.double().cpu().numpy() - w).max())
            e_t = float(np.abs(sd[i][name].double().cpu().numpy() - w).max())
            assert e_k <= allowed(e_t, float(np.abs(w).max())), (label, name, i, e_k, e_t)
    last = states[-1]
    assert last["step"] == last["applied"] == STEPS and last["gated"] == last["nonfinite"] == last["stopped"] == 0


# ---------------------------------------------------------------------------------------------------
SENTINEL = -77.0


def placed(arrays, lead):
    """Each array inside a buffer of its own, `lead` floats in, sentinels in front and behind."""
    import torch
    bufs, views = [], []
    for x in arrays:
        buf = torch.full((x.size + 12,), SENTINEL, dtype=torch.float32, device=DEV)
        view = buf[lead:lead + x.size].view(x.shape)
        view.copy_(torch.from_numpy(x))
        bufs.append(buf)
        views.append(view)
    return bufs, views


def untouched(bufs, views, lead):
    import torch
    for buf, view in zip(bufs, views):
        n = view.numel()
        assert torch.all(buf[:lead] == SENTINEL) and torch.all(buf[lead + n:] == SENTINEL)


def run_placed(params, grads, lead_p, lead_g, lead_m):
    """Three steps with every parameter, gradient and the two arenas `lead` floats into sentinel-filled
    buffers (lead 4: 16-byte aligned; lead 1: 4-byte aligned only).  Returns the bits of the parameters,
    the moments and the norms."""
    import torch
    from splendor_gym.ppo import DeviceAdam
    p_bufs, p = placed(params, lead_p)
    opt = DeviceAdam(p, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
    arenas = []
    for _ in range(2):
        buf = torch.full((opt.arena_floats + 12,), SENTINEL, dtype=torch.float32, device=DEV)
        arenas.append((buf, buf[lead_m:lead_m + opt.arena_floats]))
    opt._place_arenas(arenas[0][1], arenas[1][1])
    for arena in (opt._exp_avg, opt._exp_avg_sq):
        for seg in opt._moments(arena):
            seg.zero_()  # the padding between two segments keeps its sentinel
    assert (p[0].data_ptr() % 16 == 0) == (lead_p == 4) and (opt._exp_avg.data_ptr() % 16 == 0) == (lead_m == 4)
    norms = []
    for g in grads:
        g_bufs, gv = placed(g, lead_g)
        assert (gv[0].data_ptr() % 16 == 0) == (lead_g == 4)
        give(p, gv)
        opt.step()
        norms.append(opt.read_state()["grad_norm"])
        untouched(g_bufs, gv, lead_g)
        assert all(torch.equal(v.cpu(), torch.from_numpy(x)) for v, x in zip(gv, g))  # gradients are read only
    untouched(p_bufs, p, lead_p)
    for buf, arena in arenas:
        untouched([buf], [arena], lead_m)
        inside = torch.ones(opt.arena_floats, dtype=torch.bool, device=DEV)
        for at, x in zip(opt._at, p):
            inside[at:at + x.numel()] = False
        assert torch.all(arena[inside] == SENTINEL)  # the padding
    assert opt.read_state()["step"] == len(grads)
    return bits(p) + bits(opt._moments(opt._exp_avg)) + bits(opt._moments(opt._exp_avg_sq)), norms


@pytest.fixture(scope="module")
def aligned_run():
    C = chunk()
    shapes = ((5,), (C + 1,), (2 * C + 3,), (4,), (1,), (3, 7))
    params, grads = make_problem(shapes, 21, 3)
    return params, grads, run_placed(params, grads, 4, 4, 4)


@pytest.mark.parametrize("leads", [(1, 1, 1), (4, 1, 4), (4, 4, 1), (1, 4, 4)], ids=["all", "gradients", "arenas", "parameters"])
def test_unaligned_segments_give_the_same_bits(aligned_run, leads):
    """[1:]-style views (4-byte but not 16-byte aligned) of parameters, gradients or arenas take the dword
    path: the same bits as the aligned run, and nothing written outside any segment."""
    import torch
    params, grads, (want, want_norms) = aligned_run
    got, norms = run_placed(params, grads, *leads)
    assert norms == want_norms
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_two_runs_give_the_same_bytes():
    import torch
    params, grads = make_problem(AGENT_SHAPES, 31, 3)
    seen = []
    for _ in range(2):
        p, opt, states = run_device(params, grads)
        seen.append((bits(p) + bits([opt._exp_avg, opt._exp_avg_sq]), [s["grad_norm"] for s in states]))
    assert seen[0][1] == seen[1][1]
    assert all(torch.equal(a, b) for a, b in zip(seen[0][0], seen[1][0]))


# ---------------------------------------------------------------------------------------------------
def loss_out_of(k, kl):
    """A PPOLossOut whose fields tell call k apart (approx_kl = kl)."""
    import torch
    from splendor_gym.ppo import PPOLossOut
    vals = [k + 0.125, k + 0.25, k + 0.375, k + 0.5, kl, k + 0.75]
    buf = torch.tensor(vals + [0.0], dtype=torch.float64, device=DEV)
    buf.view(torch.int32)[13] = k  # bad
    return PPOLossOut(buf, torch), {**dict(zip(STATS, vals)), "bad": k}


@pytest.mark.parametrize("via", ["approx_kl64", "approx_kl32", "loss_out"])
def test_gate_follows_the_oracle(via):
    """KL_EPOCHS through step(): active, applied, gated and stopped after each call equal the oracle's (which
    test_ppo_adam_host pins to a loop with `break`), a gated call changes no bit, begin_epoch re-arms, and
    first / last hold the loss_out of the first / latest applied call."""
    import torch
    from splendor_gym.ppo import DeviceAdam
    want, _ = gate_sequence(KL_EPOCHS, TARGET_KL)
    params, grads = make_problem(((5,), (2051,)), 41, 1)
    p = on_device(params)
    opt = DeviceAdam(p, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, target_kl=0.0)
    opt.set_target_kl(TARGET_KL)
    g = on_device(grads[0])
    snapshot = lambda: bits(p) + bits([opt._exp_avg, opt._exp_avg_sq])
    opt.begin_update()
    k, first, last, steps = 0, None, None, 0
    for e, kls in enumerate(KL_EPOCHS):
        if e:
            opt.begin_epoch()
            assert opt.read_state()["stopped"] == 0
        for kl in kls:
            give(p, g)
            before = snapshot()
            out, fields = loss_out_of(k, kl if via == "loss_out" else 9.0)  # 9.0: ignored when approx_kl is given
            if via == "loss_out":
                opt.step(loss_out=out)
            else:
                dt = torch.float64 if via == "approx_kl64" else torch.float32
                opt.step(loss_out=out, approx_kl=torch.tensor(kl, dtype=dt, device=DEV))
            st = opt.read_state()
            assert (st["active"], st["applied"], st["gated"], st["stopped"]) == want[k], (k, st)
            if st["active"]:
                steps += 1
                last = fields
                first = first or fields
                assert not all(torch.equal(a, b) for a, b in zip(before, snapshot()))
            else:
                assert all(torch.equal(a, b) for a, b in zip(before, snapshot()))
            assert st["step"] == steps and st["first"] == first and st["last"] == last
            k += 1
    assert steps == 5 and opt.read_state()["gated"] == 4
    opt.begin_update()
    st = opt.read_state()
    assert st["applied"] == st["gated"] == st["nonfinite"] == st["stopped"] == 0 and st["step"] == 5
    assert st["first"] == {**dict.fromkeys(STATS, 0.0), "bad": 0} and st["last"] == last


@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_gradient_is_skipped(poison):
    import torch
    from splendor_gym.ppo import DeviceAdam
    C = chunk()
    params, grads = make_problem(((7,), (C + 9,)), 51, 2)
    p = on_device(params)
    opt = DeviceAdam(p, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
    give(p, on_device(grads[0]))
    opt.step()
    before = bits(p) + bits([opt._exp_avg, opt._exp_avg_sq])
    bad = [x.copy() for x in grads[1]]
    bad[1][C + 3] = poison  # in the second chunk of the second segment
    give(p, on_device(bad))
    opt.step()
    st = opt.read_state()
    assert st["nonfinite"] == 1 and st["active"] == 0 and st["step"] == st["applied"] == 1 and st["gated"] == 0
    assert not np.isfinite(st["grad_norm"])
    assert all(torch.equal(a, b) for a, b in zip(before, bits(p) + bits([opt._exp_avg, opt._exp_avg_sq])))
    give(p, on_device(grads[1]))
    opt.step()
    st = opt.read_state()
    assert st["nonfinite"] == 1 and st["active"] == 1 and st["step"] == st["applied"] == 2
    # the two finite calls are steps 1 and 2 of the oracle
    state = adam_state(lr=LR, eps=EPS, max_norm=MAX_NORM)
    want, _, _, _ = run_oracle(params, grads, state)
    ref, _, _ = run_torch(params, grads)
    compare("after a non-finite call", p, ref, want, 2)


def test_captured_step_follows_set_lr():
    """One step() captured as a single-stream graph (after an eager call on a side stream) and replayed
    three times with set_lr between the replays: bit-equal to four eager calls with those rates, so no
    hyper-parameter was baked into the capture."""
    import torch
    from splendor_gym.ppo import DeviceAdam
    rates = (LR, 1e-3, 5e-5, 2e-4)
    params, grads = make_problem(((300,), (2 * chunk() + 3,)), 61, 1)
    g = on_device(grads[0])
    # eager
    p_e = on_device(params)
    eager = DeviceAdam(p_e, lr=rates[0], eps=EPS, max_grad_norm=MAX_NORM)
    for k, lr in enumerate(rates):
        if k:
            eager.set_lr(lr)
        give(p_e, g)
        eager.step()
    # captured
    p_g = on_device(params)
    opt = DeviceAdam(p_g, lr=rates[0], eps=EPS, max_grad_norm=MAX_NORM)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        give(p_g, g)
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        give(p_g, g)
        opt.step()
    assert opt.read_state()["step"] == 1  # capturing ran nothing
    for lr in rates[1:]:
        opt.set_lr(lr)
        graph.replay()
    torch.cuda.synchronize()
    a, b = eager.read_state(), opt.read_state()
    assert a["step"] == b["step"] == 4 and a["lr"] == b["lr"] == rates[-1] and a["grad_norm"] == b["grad_norm"]
    got = bits(p_g) + bits([opt._exp_avg, opt._exp_avg_sq])
    want = bits(p_e) + bits([eager._exp_avg, eager._exp_avg_sq])
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    # and the rates mattered: the same four calls at one rate end elsewhere
    p_c = on_device(params)
    const = DeviceAdam(p_c, lr=rates[0], eps=EPS, max_grad_norm=MAX_NORM)
    for _ in rates:
        give(p_c, g)
        const.step()
    assert not torch.equal(p_c[1], p_e[1])


def test_checkpoints_in_torchs_format():
    """torch.optim.Adam for three steps, its state_dict loaded into a DeviceAdam, a fourth step on both: within
    the tolerance of the float64 oracle's four steps.  DeviceAdam's own state_dict has torch's keys and shapes,
    torch loads it, and a save / load round trip is bit-exact."""
    import torch
    from splendor_gym.ppo import DeviceAdam
    shapes = ((256, 45), (45,), (2051,), (1,))
    params, grads = make_problem(shapes, 71, 4)
    state = adam_state(lr=LR, eps=EPS, max_norm=MAX_NORM)
    want, _, _, _ = run_oracle(params, grads, state)
    ref, ref_opt, _ = run_torch(params, grads[:3])
    sd3 = copy.deepcopy(ref_opt.state_dict())
    p = [x.detach().clone() for x in ref]
    opt = DeviceAdam(p, lr=1.0, betas=(0.5, 0.5), eps=1.0, max_grad_norm=MAX_NORM)  # the group's values replace these
    opt.load_state_dict(sd3)
    st = opt.read_state()
    assert (st["step"], st["lr"], st["beta1"], st["beta2"], st["eps"]) == (3, LR, 0.9, 0.999, EPS)
    for i in range(len(shapes)):
        assert torch.equal(opt._moments(opt._exp_avg)[i], sd3["state"][i]["exp_avg"])
        assert torch.equal(opt._moments(opt._exp_avg_sq)[i], sd3["state"][i]["exp_avg_sq"])
    g4 = on_device(grads[3])
    give(ref, [x.clone() for x in g4])
    torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
    ref_opt.step()
    give(p, g4)
    opt.step()
    compare("torch x 3 + device x 1", p, ref, want, 4)
    # the format
    mine, theirs = opt.state_dict(), ref_opt.state_dict()
    assert set(mine) == set(theirs) and set(mine["state"]) == set(theirs["state"])
    assert [set(x) for x in mine["param_groups"]] == [set(x) for x in theirs["param_groups"]]
    for i in range(len(shapes)):
        assert set(mine["state"][i]) == set(theirs["state"][i])
        for key in theirs["state"][i]:
            a, b = mine["state"][i][key], theirs["state"][i][key]
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, (i, key)
        assert float(mine["state"][i]["step"]) == 4.0
    torch.optim.Adam([torch.nn.Parameter(x.clone()) for x in p], lr=LR).load_state_dict(mine)
    # round trip
    p2 = [x.clone() for x in p]
    opt2 = DeviceAdam(p2, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
    opt2.load_state_dict(mine)
    assert all(torch.equal(a, b) for a, b in zip(bits([opt._exp_avg, opt._exp_avg_sq]), bits([opt2._exp_avg, opt2._exp_avg_sq])))
    assert opt2.read_state()["step"] == 4
    for o, q in ((opt, p), (opt2, p2)):
        give(q, g4)
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(bits(p), bits(p2)))
    # a fresh optimiser's state_dict is torch's empty one, and loads
    fresh = DeviceAdam(p2, lr=LR, eps=EPS).state_dict()
    assert fresh["state"] == {} and fresh["param_groups"][0]["lr"] == LR
    opt2.load_state_dict(fresh)
    assert opt2.read_state()["step"] == 0 and not opt2._exp_avg.any() and not opt2._exp_avg_sq.any()


def test_constructor_and_step_refusals():
    import torch
    from splendor_gym.ppo import DeviceAdam, PPOLossOut
    ok = lambda *shape: torch.zeros(*shape, device=DEV)
    for bad in ([], [ok(2)] * 17, [ok(2).double()], [ok(4, 4).t()], [ok(0)], [torch.zeros(2)], [ok(2), torch.zeros(2)], [3.0]):
        with pytest.raises(ValueError):
            DeviceAdam(bad)
    p = [ok(4, 4), ok(3)]
    opt = DeviceAdam(p)
    with pytest.raises(ValueError, match="no gradient"):
        opt.step()
    p[0].grad, p[1].grad = ok(4, 4).t(), ok(3)  # torch itself lets a non-contiguous gradient in
    with pytest.raises(ValueError, match="gradient of parameter 0"):
        opt.step()

    class Holder:  # stands in for a parameter: torch polices the dtype, shape and device of a real one's .grad
        def __init__(self, x, g):
            self.x, self.grad = x, g

        def __getattr__(self, name):
            return getattr(self.x, name)

    for g in (ok(4, 4).double(), ok(4, 4).t(), ok(16), torch.zeros(4, 4)):
        opt.params = [Holder(p[0], g), Holder(p[1], ok(3))]
        with pytest.raises(ValueError, match="gradient of parameter 0"):
            opt.step()
    opt.params = p
    give(p, [ok(4, 4), ok(3)])
    for kl in (0.5, torch.zeros(2, device=DEV), torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="approx_kl"):
            opt.step(approx_kl=kl)
    with pytest.raises(ValueError, match="loss_out"):
        opt.step(loss_out=torch.zeros(7, dtype=torch.float64, device=DEV))
    assert opt.read_state()["step"] == 0 and p[0].grad is not None  # nothing was launched, nothing taken
    opt.step(loss_out=PPOLossOut(torch.zeros(7, dtype=torch.float64, device=DEV), torch))
    assert opt.read_state()["step"] == 1 and p[0].grad is None


# ---------------------------------------------------------------------------------------------------
def update_f64(agent, store, epochs, minibatch, target_kl, seed=0):
    """ppo_update's torch head on a float64 copy of the agent with clip_grad_norm_ + torch.optim.Adam in float64
    (default coefficients, the reference's `break`).  Returns the parameters, the KL of every minibatch that
    ran and the number of optimiser steps."""
    import torch
    a = copy.deepcopy(agent).double()
    opt = torch.optim.Adam(a.parameters(), lr=LR, eps=EPS)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    d = lambda x: x.double()
    kls = []
    for _ in range(epochs):
        for idx in store.minibatches(minibatch, gen):
            mb = store.gather(idx, normalize=True)
            _, new_logprob, entropy, new_value = a.get_action_and_value(d(mb["obs"]), mb["mask"], mb["action"])
            ratio = (new_logprob - d(mb["logprob"])).exp()
            clip_adv = torch.clamp(ratio, 1 - 0.2, 1 + 0.2) * d(mb["adv"])
            policy_loss = -torch.min(ratio * d(mb["adv"]), clip_adv).mean()
            v_pred = new_value.squeeze(-1)
            v_clipped = d(mb["value"]) + torch.clamp(v_pred - d(mb["value"]), -0.2, 0.2)
            value_loss = 0.5 * torch.max((v_pred - d(mb["ret"])).pow(2), (v_clipped - d(mb["ret"])).pow(2)).mean()
            loss = policy_loss + 0.5 * value_loss + 0.03 * entropy.mean()
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(a.parameters(), MAX_NORM)
            opt.step()
            kls.append(float((d(mb["logprob"]) - new_logprob).mean().detach()))
            if target_kl > 0 and kls[-1] > target_kl:
                break
    return list(a.parameters()), kls, len(kls)


def run_update(agent, store, device_adam, target_kl, **switches):
    """ppo_update on a copy of the agent, two epochs of minibatches of 64 from generator seed 0, with either optimiser.
    switches: ppo_update's own (fused_loss=True unless given), or tiled=... for a DeviceNets(copy, tiled=...) as
    device_nets.  Returns the parameters, the dictionary and the optimiser."""
    import torch
    from splendor_gym.ppo import DeviceAdam, DeviceNets, ppo_update
    a = copy.deepcopy(agent)
    make = DeviceAdam if device_adam else torch.optim.Adam
    opt = make(list(a.parameters()), lr=LR, eps=EPS)
    gen = torch.Generator(device=DEV).manual_seed(0)
    switches.setdefault("fused_loss", True)
    if "tiled" in switches:
        switches["device_nets"] = DeviceNets(a, tiled=switches.pop("tiled"))
    res = ppo_update(a, opt, store, update_epochs=2, minibatch_size=64, target_kl=target_kl, generator=gen, **switches)
    return list(a.parameters()), res, opt


@pytest.fixture(scope="module")
def reference_update(collected):
    """The float64 update without a gate, shared by the tests below and by those of test_gpu_ppo_net.py (nothing
    changes it)."""
    agent, store = collected
    return update_f64(agent, store, 2, 64, 0.0)


def choose_target_kl(agent, store, kls):
    """target_kl: a midpoint between two neighbours among the ungated run's own minibatch KLs, chosen by the float64
    loop with `break`: of the midpoints from which every KL of the gated float64 run stays well away, the one that
    stops it earliest.  Returns the count the float64 loop stops at, the target and e32.

    float32 KLs must fall on the float64 ones' side of the target: the margin is set against the float32 torch
    path's own distance from the float64 loop (e32), measured on the ungated run's last minibatch."""
    e32 = abs(run_update(agent, store, False, 0.0)[1]["approx_kl"] - kls[-1])
    print(f"minibatch KLs {['%.3e' % k for k in kls]}; float32 torch path against the float64 loop, last KL: {e32:.3e}")
    s, best = sorted(kls), None
    for a, b in zip(s, s[1:]):
        if a + b > 0:
            target = (a + b) / 2
            _, ran, n = update_f64(agent, store, 2, 64, target)
            margin = min(abs(k - target) for k in ran)
            print(f"target {target:.3e}: the float64 loop takes {n} steps, nearest KL {margin:.3e} away")
            if margin > 100 * e32 and margin > 1e-3 * target and (best is None or n < best[0]):
                best = (n, target)
    assert best is not None and best[0] < 8  # the gate acts
    return best[0], best[1], e32


def test_ppo_update_with_the_optimiser_on_the_device(collected, reference_update):
    agent, store = collected
    want, kls, steps = reference_update
    assert steps == 8
    want = [x.detach().cpu().numpy() for x in want]
    p_dev, res_dev, opt = run_update(agent, store, True, 0.0)
    p_ref, res_ref, _ = run_update(agent, store, False, 0.0)
    assert res_dev["optimizer_steps"] == res_ref["optimizer_steps"] == 8 and res_dev["gated"] == 0
    compare("ppo_update", p_dev, p_ref, want, 8)
    assert set(res_dev) == set(res_ref) | {"gated", "grad_norm"}
    for name in ("policy_loss", "value_loss", "entropy", "approx_kl", "first_approx_kl", "clipfrac"):
        print(f"ppo_update {name}: device {res_dev[name]:+.6e} torch {res_ref[name]:+.6e}")
        assert np.isfinite(res_dev[name])
    for name, w in (("approx_kl", kls[-1]), ("first_approx_kl", kls[0])):
        assert abs(res_dev[name] - w) <= allowed(abs(res_ref[name] - w), abs(w)), name
    assert np.isfinite(res_dev["grad_norm"]) and res_dev["grad_norm"] > 0
    assert opt.max_grad_norm == 0.5 and opt.target_kl == 0.0  # ppo_update's arguments
    assert all(x.grad is None for x in p_dev) and int(store.errors.item()) == 0
    # the torch head with the optimiser on the device: the same dictionary without clipfrac
    p_head, res_head, _ = run_update(agent, store, True, 0.0, fused_loss=False)
    assert res_head["optimizer_steps"] == 8 and "clipfrac" not in res_head and set(res_head) == set(res_dev) - {"clipfrac"}
    compare("ppo_update, torch head", p_head, p_ref, want, 8)


def test_ppo_update_stops_where_the_torch_path_stops(collected, reference_update):
    """With choose_target_kl's target both optimisers must stop at the count the float64 loop stops at."""
    agent, store = collected
    _, kls, _ = reference_update
    want_steps, target, e32 = choose_target_kl(agent, store, kls)
    _, res_dev, opt = run_update(agent, store, True, target)
    _, res_ref, _ = run_update(agent, store, False, target)
    assert res_dev["optimizer_steps"] == res_ref["optimizer_steps"] == want_steps
    assert res_dev["gated"] == 8 - want_steps and opt.target_kl == target
    assert abs(res_dev["approx_kl"] - res_ref["approx_kl"]) <= 100 * e32 + 1e-3 * target  # the same last applied minibatch


def run_cli(*flags, updates):
    """python -m splendor_gym.scripts.ppo_device with `flags` at a toy size (64 tables x 4 steps, minibatches of 128,
    `updates` updates from the committed checkpoint) in a child process: exit 0; returns the printed update lines."""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "splendor-gym_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg] + [x for x in (os.environ.get("PYTHONPATH"),) if x]))
    r = subprocess.run([sys.executable, "-m", "splendor_gym.scripts.ppo_device", "--num-envs", "64", "--num-steps", "4",
                        "--total-timesteps", str(updates * 64 * 4), "--minibatch-size", "128", "--pool-size", "2", *flags,
                        "--load-path", os.path.join(here, "golden", "ppo_splendor_latest.safetensors")],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("update ")]
    assert len(lines) == updates and lines[-1].startswith(f"update {updates}/{updates} steps {updates * 256} "), r.stdout[-2000:]
    return lines


def finite_figures(line, most_steps):
    nums = re.findall(r"(?:pl|vl|ent|kl) ([-+0-9.einfa]+)", line)
    assert len(nums) == 4 and all(np.isfinite(float(x)) for x in nums), line
    assert 1 <= int(re.search(r"opt-steps (\d+)", line).group(1)) <= most_steps, line


def test_cli_device_adam():
    """ppo_device --device-adam --fused-loss: two updates, every printed figure finite."""
    for ln in run_cli("--update-epochs", "2", "--fused-loss", "--device-adam", "--lr-anneal", updates=2):
        finite_figures(ln, 4)
