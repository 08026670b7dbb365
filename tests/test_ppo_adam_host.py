"""The PPO optimiser step without a GPU (spl_ppo_adam, include/splendor_ppo.h): the numpy float64 oracle the
GPU tests compare against, pinned to torch's clip_grad_norm_ + Adam in float64 on the CPU and to a literal
loop with `break` for the target-KL gate; the struct layouts against the header; every host-side refusal
of the entry points; and the state_dict format against torch.optim.Adam's own."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

# the agent's layer shapes: both first layers' kind, a hidden layer, the actor's and the critic's outputs
SHAPES = ((256, 297), (256,), (256, 256), (256,), (45, 256), (45,), (1, 256), (1,))
SCALES = (3.0, 1e-3, 0.05, 10.0, 1e-6, 0.3)  # gradient scales: norms far above and far below max_norm = 0.5
STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac")
# three epochs of minibatch KLs, target 0.02: the second call of epoch 1 and the first of epoch 3 cross it
KL_EPOCHS = ((0.01, 0.03, 0.01), (0.01, 0.01), (0.05, 0.01, 0.01, 0.03))
TARGET_KL = 0.02


def adam_state(lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_norm=0.5, target_kl=0.0):
    """A fresh spl_ppo_adam_state_t as a dict."""
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm, target_kl=target_kl, step=0, applied=0,
                gated=0, nonfinite=0, stopped=0, active=0, grad_norm=0.0, clip_coef=0.0, first=None, last=None)


def adam_oracle_begin(state, update):
    """spl_ppo_adam_begin: a new epoch re-arms the gate; a new update also clears the counters and `first`."""
    state["stopped"] = 0
    if update:
        state.update(applied=0, gated=0, nonfinite=0, first=None)


def adam_oracle_step(p, g, m, v, state, approx_kl=None, loss_out=None):
    """One spl_ppo_adam call in float64 on lists of arrays (p, m, v are replaced in the lists when the call
    is active, `state` is updated in place): rules 1 to 5 of include/splendor_ppo.h with every float32
    rounding left out.  loss_out: any object to latch; a dict with "approx_kl" supplies the KL when
    approx_kl is None."""
    with np.errstate(all="ignore"):
        norm = math.sqrt(sum(float((np.asarray(x, dtype=np.float64) ** 2).sum()) for x in g))
        mx = state["max_norm"]
        cn = mx / (norm + 1e-6)
        coef = 1.0 if mx < 0 else (cn if cn < 1.0 else 1.0)
    state["grad_norm"], state["clip_coef"] = norm, coef
    armed, finite = not state["stopped"], math.isfinite(norm)
    state["active"] = int(armed and finite)
    if not armed:
        state["gated"] += 1
    elif not finite:
        state["nonfinite"] += 1
    else:
        state["step"] += 1
        if loss_out is not None:
            state["last"] = loss_out
            if state["applied"] == 0:
                state["first"] = loss_out
        state["applied"] += 1
    kl = approx_kl if approx_kl is not None else (loss_out["approx_kl"] if isinstance(loss_out, dict) else None)
    if state["target_kl"] > 0 and kl is not None and kl > state["target_kl"]:
        state["stopped"] = 1
    if not state["active"]:
        return
    b1, b2, t = state["beta1"], state["beta2"], state["step"]
    step_size, bc2_sqrt = state["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
    for i in range(len(p)):
        gc = np.asarray(g[i], dtype=np.float64) * coef
        m[i] = m[i] + (gc - m[i]) * (1.0 - b1)
        v[i] = v[i] * b2 + (1.0 - b2) * (gc * gc)
        p[i] = p[i] - step_size * (m[i] / (np.sqrt(v[i]) / bc2_sqrt + state["eps"]))


def make_problem(shapes, seed, steps=len(SCALES)):
    """float32 parameters and one float32 gradient per step and tensor, scaled by SCALES in turn."""
    rng = np.random.default_rng(seed)
    params = [(0.1 * rng.normal(size=s)).astype(np.float32) for s in shapes]
    grads = [[(SCALES[k % len(SCALES)] * rng.normal(size=s) / math.sqrt(sum(int(np.prod(x)) for x in shapes))).astype(np.float32)
              for s in shapes] for k in range(steps)]
    return params, grads


def run_oracle(params, grads, state, kls=None):
    """The oracle over all steps from zero moments; returns p, m, v and the (norm, coef, active) of each call."""
    p = [x.astype(np.float64) for x in params]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    calls = []
    for k, g in enumerate(grads):
        adam_oracle_step(p, g, m, v, state, approx_kl=None if kls is None else kls[k])
        calls.append((state["grad_norm"], state["clip_coef"], state["active"]))
    return p, m, v, calls


@pytest.mark.parametrize("max_norm", [0.5, None])
def test_oracle_equals_torch_in_float64(max_norm):
    """clip_grad_norm_(., 0.5) + Adam(lr=2.5e-4, eps=1e-5) in float64 on the CPU, six steps whose norms lie
    on both sides of 0.5: 1e-14 absolute in the parameters, 1e-13 relative in the norm (measured: 5.6e-17
    and 2.0e-14, two summation orders over 296 000 squares).  With max_norm off the
    oracle is Adam alone."""
    import torch
    params, grads = make_problem(SHAPES, 1)
    state = adam_state(max_norm=-1.0 if max_norm is None else max_norm)
    p, m, v, calls = run_oracle(params, grads, state)
    tp = [torch.nn.Parameter(torch.from_numpy(x.astype(np.float64))) for x in params]
    opt = torch.optim.Adam(tp, lr=2.5e-4, eps=1e-5)
    norms = []
    for g in grads:
        for x, gi in zip(tp, g):
            x.grad = torch.from_numpy(gi.astype(np.float64))
        if max_norm is None:
            norms.append(float(torch.cat([x.grad.reshape(-1) for x in tp]).norm()))
        else:
            norms.append(float(torch.nn.utils.clip_grad_norm_(tp, max_norm)))
        opt.step()
    e_p = max(float(np.abs(a - b.detach().numpy()).max()) for a, b in zip(p, tp))
    e_n = max(abs(c[0] - n) / n for c, n in zip(calls, norms))
    print(f"oracle against torch float64: parameters {e_p:.3e} norm (relative) {e_n:.3e}")
    assert e_p <= 1e-14 and e_n <= 1e-13
    coefs = [c[1] for c in calls]
    if max_norm is None:
        assert coefs == [1.0] * len(grads)
    else:
        assert min(coefs) < 0.5 and max(coefs) == 1.0  # clipped and unclipped calls both occur
    sd = opt.state_dict()["state"]
    assert max(float(np.abs(a - sd[i]["exp_avg"].numpy()).max()) for i, a in enumerate(m)) <= 1e-14
    assert max(float(np.abs(a - sd[i]["exp_avg_sq"].numpy()).max()) for i, a in enumerate(v)) <= 1e-14
    assert state["step"] == state["applied"] == len(grads) and state["gated"] == state["nonfinite"] == 0


def literal_loop(epochs, target):
    """ppo_splendor.py:354-361 as written: step, then `break` out of the epoch when the KL is above the
    target.  Returns, per minibatch in order, whether its step was taken."""
    taken = []
    for kls in epochs:
        stepped = [False] * len(kls)
        for i, kl in enumerate(kls):
            stepped[i] = True  # optimizer.step()
            if target > 0 and kl > target:
                break
        taken += stepped
    return taken


def gate_sequence(epochs, target):
    """The oracle fed every minibatch of every epoch: (active, applied, gated, stopped) after each call."""
    state = adam_state(target_kl=target)
    p, g = [np.ones(3)], [np.full(3, 0.1)]
    m, v = [np.zeros(3)], [np.zeros(3)]
    seen = []
    adam_oracle_begin(state, update=True)
    for e, kls in enumerate(epochs):
        if e:
            adam_oracle_begin(state, update=False)
        for kl in kls:
            adam_oracle_step(p, g, m, v, state, approx_kl=kl)
            seen.append((state["active"], state["applied"], state["gated"], state["stopped"]))
    return seen, state


@pytest.mark.parametrize("target", [TARGET_KL, 0.0, 0.04])
def test_gate_equals_a_loop_with_break(target):
    taken = literal_loop(KL_EPOCHS, target)
    seen, state = gate_sequence(KL_EPOCHS, target)
    assert [bool(s[0]) for s in seen] == taken
    assert state["applied"] == state["step"] == sum(taken) and state["gated"] == len(taken) - sum(taken)
    if target == TARGET_KL:
        assert taken == [True, True, False, True, True, True, False, False, False]
        assert [s[3] for s in seen] == [0, 1, 1, 0, 0, 1, 1, 1, 1]
    if target == 0.0:
        assert all(taken) and state["stopped"] == 0


def test_oracle_skips_leave_everything_and_latch_first_and_last():
    state = adam_state(target_kl=TARGET_KL)
    p, m, v = [np.ones(4)], [np.zeros(4)], [np.zeros(4)]
    adam_oracle_begin(state, update=True)
    out = lambda kl: {"approx_kl": kl}
    adam_oracle_step(p, [np.array([0.1, np.inf, 0.0, 0.0])], m, v, state, loss_out=out(0.0))
    assert state["nonfinite"] == 1 and state["step"] == 0 and state["first"] is None and (p[0] == 1).all()
    adam_oracle_step(p, [np.array([0.1, np.nan, 0.0, 0.0])], m, v, state, loss_out=out(0.0))
    assert state["nonfinite"] == 2 and state["active"] == 0
    a, b, c = out(0.001), out(0.5), out(0.002)
    adam_oracle_step(p, [np.full(4, 0.1)], m, v, state, loss_out=a)
    adam_oracle_step(p, [np.full(4, 0.1)], m, v, state, loss_out=b)  # its KL crosses the line: applied, then latched
    assert state["step"] == 2 and state["stopped"] == 1 and state["first"] is a and state["last"] is b
    before = (p[0].copy(), m[0].copy(), v[0].copy())
    adam_oracle_step(p, [np.full(4, 0.1)], m, v, state, loss_out=c)
    assert state["gated"] == 1 and state["step"] == 2 and state["last"] is b
    assert all(np.array_equal(x, y) for x, y in zip(before, (p[0], m[0], v[0])))
    adam_oracle_begin(state, update=False)
    adam_oracle_step(p, [np.full(4, 0.1)], m, v, state, loss_out=c)
    assert state["step"] == 3 and state["last"] is c and state["first"] is a and state["gated"] == 1
    adam_oracle_begin(state, update=True)
    assert state["first"] is None and state["applied"] == state["gated"] == state["nonfinite"] == 0 and state["step"] == 3


# --------------------------------------------------------------------------------------------
P = 0x10000  # a plausible, aligned, never-dereferenced device address: every case below is refused first


def _lib():
    from splendor_gym import _native
    return _native, _native.load_library()  # dlopen only: no GPU needed


def _refused(lib, code, word):
    assert code < 0, code
    msg = lib.spl_last_error()
    assert msg and word.encode() in msg, msg


def header_fields(src, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [re.sub(r"\[.*\]", "", x.strip().split()[-1]).strip("*") for x in [first] + rest]
    return fields


def test_struct_layouts_against_the_header():
    native, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splendor_ppo.h")).read()
    assert re.search(r"#define SPL_PPO_ABI 1\b", src) and lib.spl_abi_version() == 9  # additive: neither moved
    for macro, value in (("SPL_PPO_ADAM", 1), ("SPL_PPO_ADAM_MAX_TENSORS", native.PPO_ADAM_MAX_TENSORS),
                         ("SPL_PPO_ADAM_CHUNK", native.PPO_ADAM_CHUNK), ("SPL_PPO_ADAM_PARTS", native.PPO_ADAM_PARTS),
                         ("SPL_PPO_ADAM_EPOCH", native.PPO_ADAM_EPOCH), ("SPL_PPO_ADAM_UPDATE", native.PPO_ADAM_UPDATE)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    assert native.PPO_ADAM_MAX_TENSORS == 16 and native.PPO_ADAM_CHUNK % 1024 == 0
    S, A = native.PpoAdamState, native.PpoAdam
    assert header_fields(src, "spl_ppo_adam_state_t") == [f[0] for f in S._fields_]
    assert header_fields(src, "spl_ppo_adam_t") == [f[0] for f in A._fields_]
    assert ctypes.sizeof(S) == 232 and ctypes.sizeof(S) % 8 == 0
    offsets = {k: getattr(S, k).offset for k in ("lr", "target_kl", "step", "applied", "gated", "nonfinite", "stopped",
                                                 "active", "grad_norm", "clip_coef", "first", "last", "step_in", "armed")}
    assert offsets == {"lr": 0, "target_kl": 40, "step": 48, "applied": 56, "gated": 64, "nonfinite": 72, "stopped": 80,
                       "active": 84, "grad_norm": 88, "clip_coef": 96, "first": 104, "last": 160, "step_in": 216, "armed": 224}
    assert ctypes.sizeof(A) == 8 + 3 * 16 * 8 + 6 * 8
    assert (A.param.offset, A.grad.offset, A.numel.offset, A.exp_avg.offset, A.scratch.offset) == (8, 136, 264, 392, 432)
    assert ctypes.sizeof(native.PpoLossOut) == 56 and ctypes.sizeof(native.PpoLoss) == 4 * 4 + 10 * 8 + 4 * 4 + 5 * 8  # unchanged


def test_scratch_bytes():
    native, lib = _lib()
    C, parts = native.PPO_ADAM_CHUNK, native.PPO_ADAM_PARTS
    # a partial sum per chunk, had every segment but one a single element; 512 at the most
    want = lambda total: min((total + C - 1) // C + 15, parts) * 8
    for total in (1, C, C + 1, 295982, parts * C, 1 << 31):
        assert lib.spl_ppo_adam_scratch_bytes(total) == want(total), total
    assert lib.spl_ppo_adam_scratch_bytes(295982) == 160 * 8 and lib.spl_ppo_adam_scratch_bytes(1 << 31) == 4096
    for total in (0, -1, -(1 << 40)):
        assert lib.spl_ppo_adam_scratch_bytes(total) < 0 and b"positive" in lib.spl_last_error()
    assert lib.spl_ppo_adam_scratch_bytes((1 << 31) + 1) < 0 and b"2^31" in lib.spl_last_error()


def adam_args(native, n=2, numel=(5, 7), **kw):
    a = native.PpoAdam(n=n, reserved=0, exp_avg=P, exp_avg_sq=P, state=P, scratch=P)
    for i in range(min(n, 16) if n > 0 else 0):
        a.param[i], a.grad[i], a.numel[i] = P, P, numel[i] if i < len(numel) else 1
    for k, val in kw.items():
        if isinstance(val, tuple):  # (index, value) of an array field
            getattr(a, k)[val[0]] = val[1]
        else:
            setattr(a, k, val)
    return ctypes.byref(a)


def test_adam_refusals():
    native, lib = _lib()
    _refused(lib, lib.spl_ppo_adam(None, None), "null")
    for n in (0, -1, 17):
        _refused(lib, lib.spl_ppo_adam(adam_args(native, n=n), None), "n must")
    _refused(lib, lib.spl_ppo_adam(adam_args(native, reserved=1), None), "reserved")
    for name in ("exp_avg", "exp_avg_sq", "state", "scratch"):
        _refused(lib, lib.spl_ppo_adam(adam_args(native, **{name: None}), None), "null")
    for name in ("param", "grad"):
        for i in (0, 1):
            _refused(lib, lib.spl_ppo_adam(adam_args(native, **{name: (i, None)}), None), "null")
            for off in (1, 2, 3):
                _refused(lib, lib.spl_ppo_adam(adam_args(native, **{name: (i, P + off)}), None), "aligned")
    for name in ("exp_avg", "exp_avg_sq"):
        for off in (1, 2, 3):
            _refused(lib, lib.spl_ppo_adam(adam_args(native, **{name: P + off}), None), "aligned")
    for name in ("state", "scratch", "approx_kl", "loss_out"):
        _refused(lib, lib.spl_ppo_adam(adam_args(native, **{name: P + 4}), None), "aligned")
    for bad in (0, -3):
        _refused(lib, lib.spl_ppo_adam(adam_args(native, numel=(5, bad)), None), "positive")
    _refused(lib, lib.spl_ppo_adam(adam_args(native, numel=((1 << 31) - 4, 5)), None), "2^31")
    _refused(lib, lib.spl_ppo_adam(adam_args(native, numel=(1 << 40, 5)), None), "2^31")
    _refused(lib, lib.spl_ppo_adam(adam_args(native, n=16, numel=(1 << 31,)), None), "2^31")


def test_begin_refusals():
    native, lib = _lib()
    _refused(lib, lib.spl_ppo_adam_begin(None, native.PPO_ADAM_EPOCH, None), "null")
    _refused(lib, lib.spl_ppo_adam_begin(P + 4, native.PPO_ADAM_UPDATE, None), "aligned")
    for what in (-1, 2):
        _refused(lib, lib.spl_ppo_adam_begin(P, what, None), "SPL_PPO_ADAM_EPOCH")


# --------------------------------------------------------------------------------------------
def test_state_dict_has_torchs_format():
    """adam_state_dict (what DeviceAdam.state_dict returns) beside torch.optim.Adam's own for the same
    parameters: the same keys at every level, the same shapes and dtypes, and adam_state_of reads both."""
    import torch
    from splendor_gym.ppo import adam_state_dict, adam_state_of
    shapes = ((7, 5), (7,), (1, 7))
    tp = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate(shapes)]
    opt = torch.optim.Adam(tp, lr=2.5e-4, eps=1e-5)
    fresh = opt.state_dict()
    assert adam_state_dict(fresh, 0, [None] * 3, [None] * 3) == {"state": {}, "param_groups": fresh["param_groups"]}
    for _ in range(2):
        for x in tp:
            x.grad = torch.ones_like(x)
        opt.step()
    want = opt.state_dict()
    ms = [want["state"][i]["exp_avg"] for i in range(3)]
    vs = [want["state"][i]["exp_avg_sq"] for i in range(3)]
    got = adam_state_dict(fresh, 2, ms, vs)
    assert set(got) == set(want) and set(got["state"]) == set(want["state"])
    assert [set(g) for g in got["param_groups"]] == [set(g) for g in want["param_groups"]]
    assert got["param_groups"][0]["params"] == want["param_groups"][0]["params"] == [0, 1, 2]
    for i in range(3):
        assert set(got["state"][i]) == set(want["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in want["state"][i]:
            a, b = got["state"][i][k], want["state"][i][k]
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), (i, k)
        assert got["state"][i]["exp_avg"].data_ptr() != ms[i].data_ptr()  # a copy, not a view of the arena
    torch.optim.Adam(tp, lr=1.0).load_state_dict(got)  # torch takes it
    for sd in (got, want):
        step, m2, v2, group = adam_state_of(sd, shapes)
        assert step == 2 and group["lr"] == 2.5e-4 and group["eps"] == 1e-5 and tuple(group["betas"]) == (0.9, 0.999)
        assert all(torch.equal(a, b) for a, b in zip(m2 + v2, ms + vs))
    assert adam_state_of(fresh, shapes)[:3] == (0, [None] * 3, [None] * 3)
    with pytest.raises(ValueError, match="shape"):
        adam_state_of(want, ((7, 5), (7,), (7, 1)))
    with pytest.raises(ValueError, match="parameters"):
        adam_state_of(want, shapes[:2])
    decayed = {**want, "param_groups": [{**want["param_groups"][0], "weight_decay": 0.01}]}
    with pytest.raises(ValueError, match="weight decay"):
        adam_state_of(decayed, shapes)
    uneven = {**want, "state": {**want["state"], 1: {**want["state"][1], "step": torch.tensor(5.0)}}}
    with pytest.raises(ValueError, match="step"):
        adam_state_of(uneven, shapes)


def test_device_adam_needs_a_gpu_or_refuses():
    """No CPU fallback: without a GPU the constructor raises; with one it refuses CPU parameters."""
    import torch
    from splendor_gym.ppo import DeviceAdam
    with pytest.raises((RuntimeError, ValueError)):
        DeviceAdam([torch.nn.Parameter(torch.zeros(4))])
