"""The PPO loss head without a GPU (spl_ppo_loss, include/splendor_ppo.h): the numpy float64 oracle the
GPU tests compare against, checked against torch.autograd on the literal expression of
splendor_gym/ppo.py's update and against a row worked by hand; the cases whose branches are fixed by
construction; and every host-side refusal of the entry point."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

NA = 45
ALL = (1 << NA) - 1
RHO = (0.5, 0.9, 1.0, 1.1, 1.5)        # ratio regimes: with clip_coef 0.2 each at least 0.1 from 0.8 and 1.2
DELTA = (-0.5, -0.1, 0.0, 0.1, 0.5)    # v - v_old regimes: with vclip 0.2 each at least 0.1 from +-0.2
COEF = dict(clip_coef=0.2, vclip=0.2, vf_coef=0.5, ent_coef=0.03)


def loss_oracle(logits, value, mask_bits, action, lp_old, v_old, adv, ret, clip_coef, vclip, vf_coef, ent_coef, bad=None):
    """include/splendor_ppo.h's spl_ppo_loss in float64, row b of every argument one minibatch row (the
    recorded planes already gathered).  ent_coef is signed.  `bad` marks rows to drop (positions outside
    the store); a row whose action is outside its legal set is dropped too.  Returns dlogits [B, 45],
    dvalue [B], the six statistics and bad (the number of dropped rows); every mean divides by B."""
    logits, value, lp_old, v_old, adv, ret = (np.asarray(x, dtype=np.float64) for x in (logits, value, lp_old, v_old, adv, ret))
    action = np.asarray(action, dtype=np.int64)
    B = logits.shape[0]
    legal = ((np.asarray(mask_bits, dtype=np.uint64)[:, None] >> np.arange(NA, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    legal[~legal.any(axis=1)] = True
    in_range = (action >= 0) & (action < NA)
    act = np.where(in_range, action, 0)
    rows = np.arange(B)
    drop = ~(in_range & legal[rows, act])
    if bad is not None:
        drop |= np.asarray(bad, dtype=bool)
    with np.errstate(all="ignore"):
        x = np.where(legal, logits, -np.inf)
        t = x - x.max(axis=1, keepdims=True)
        logp = t - np.log(np.exp(t).sum(axis=1, keepdims=True))
        p = np.exp(logp)
        logp0 = np.where(legal, logp, 0.0)
        H = -(p * logp0).sum(axis=1)
        lp = logp0[rows, act]
        r = np.exp(lp - lp_old)
        lo, hi = 1.0 - clip_coef, 1.0 + clip_coef
        s1, s2 = r * adv, np.clip(r, lo, hi) * adv
        policy = -np.minimum(s1, s2)
        g_lp = np.where(((r >= lo) & (r <= hi)) | (s1 < s2), -adv * r / B, 0.0)
        onehot = np.zeros((B, NA))
        onehot[rows, act] = 1.0
        dlogits = np.where(legal, g_lp[:, None] * (onehot - p) - (ent_coef / B) * p * (logp0 + H[:, None]), 0.0)
        d = value - v_old
        v_c = v_old + np.clip(d, -vclip, vclip)
        e1, e2 = value - ret, v_c - ret
        q1, q2 = e1 * e1, e2 * e2
        vloss = 0.5 * np.maximum(q1, q2)
        w1 = np.where(q1 > q2, 1.0, np.where(q1 < q2, 0.0, 0.5))
        dvalue = (vf_coef / B) * (w1 * e1 + (1.0 - w1) * e2 * (np.abs(d) <= vclip))
        clipped = (np.abs(r - 1.0) > clip_coef).astype(np.float64)
    keep = ~drop
    dlogits[drop] = 0.0
    dvalue[drop] = 0.0
    mean = lambda z: float(z[keep].sum() / B)
    out = {"dlogits": dlogits, "dvalue": dvalue, "policy_loss": mean(policy), "value_loss": mean(vloss), "entropy": mean(H),
           "approx_kl": mean(lp_old - lp), "clipfrac": mean(clipped), "bad": int(drop.sum())}
    out["loss"] = out["policy_loss"] + vf_coef * out["value_loss"] + ent_coef * out["entropy"]
    return out


STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac")


def make_case(K, T, seed):
    """Per-position planes of a [K][T] store plus one logits row and one critic value per position, every
    branch of the loss fixed by construction (clip_coef = vclip = 0.2).  Position q:
      mask      q % 4: no legal action, bit 44 only, all 45, a random nonzero word; the action drawn from L
      ratio     logprob = lp - log(RHO[q % 5]) with lp the float64 log-probability of the float32 logits
      adv       sign by (q // 4) % 2, |adv| in [0.2, 2]
      v - v_old DELTA[(q // 5) % 5];  ret = v -+ [0.3, 1.5] by (q // 8) % 2: never near the tie of the two
                squared errors, which for |v - v_old| = 0.5 lies 0.15 from v
    Everything is float32 (int64 mask words, int32 actions); the oracle takes them upcast."""
    rng = np.random.default_rng(seed)
    P = K * T
    bits = np.zeros(P, dtype=np.int64)
    action = np.zeros(P, dtype=np.int32)
    for q in range(P):
        kind = q % 4
        word = 0 if kind == 0 else 1 << 44 if kind == 1 else ALL if kind == 2 else int(rng.integers(1, ALL + 1))
        bits[q] = word
        choices = [j for j in range(NA) if ((word or ALL) >> j) & 1]
        action[q] = choices[int(rng.integers(len(choices)))]
    logits = (2.0 * rng.normal(size=(P, NA))).astype(np.float32)
    v = rng.normal(size=P).astype(np.float32)
    q = np.arange(P)
    legal = ((bits.astype(np.uint64)[:, None] >> np.arange(NA, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    legal[~legal.any(axis=1)] = True
    x = np.where(legal, logits.astype(np.float64), -np.inf)
    t = x - x.max(axis=1, keepdims=True)
    lp = (t - np.log(np.exp(t).sum(axis=1, keepdims=True)))[q, action]
    logprob = (lp - np.log(np.array(RHO)[q % 5])).astype(np.float32)
    adv = (np.where((q // 4) % 2 == 0, 1.0, -1.0) * rng.uniform(0.2, 2.0, size=P)).astype(np.float32)
    value = (v.astype(np.float64) - np.array(DELTA)[(q // 5) % 5]).astype(np.float32)
    value[(q // 5) % 5 == 2] = v[(q // 5) % 5 == 2]  # v - v_old = 0 exactly: the two squared errors tie
    ret = (v.astype(np.float64) + np.where((q // 8) % 2 == 0, 1.0, -1.0) * rng.uniform(0.3, 1.5, size=P)).astype(np.float32)
    return {"K": K, "T": T, "mask_bits": bits, "action": action, "logprob": logprob, "value": value, "adv": adv,
            "ret": ret, "logits": logits, "v": v}


def case_idx(P, B, seed):
    """B flat positions with duplicates: position 7 twice and the last position when there is room."""
    idx = np.random.default_rng(seed).integers(0, P, size=B).astype(np.int64)
    if B >= 5:
        idx[:3] = (7, P - 1, 7)
    return idx


def case_rows(case, idx, **coef):
    """loss_oracle's arguments for the minibatch idx of make_case's planes."""
    g = lambda name: case[name][idx]
    return dict(logits=g("logits"), value=g("v"), mask_bits=g("mask_bits"), action=g("action"), lp_old=g("logprob"),
                v_old=g("value"), adv=g("adv"), ret=g("ret"), **{**COEF, **coef})


def test_cases_are_away_from_every_branch_point():
    case = make_case(3, 70, 1)
    rows = case_rows(case, np.arange(210))
    legal = rows["mask_bits"]
    assert (legal == 0).any() and (legal == 1 << 44).any() and (legal == ALL).any()
    x = np.where(((np.where(legal == 0, ALL, legal)[:, None] >> np.arange(NA)) & 1).astype(bool), rows["logits"].astype(np.float64), -np.inf)
    lp = (x - np.log(np.exp(x).sum(axis=1, keepdims=True)))[np.arange(210), rows["action"]]
    r = np.exp(lp - rows["lp_old"])
    assert np.abs(r - np.array(RHO)[np.arange(210) % 5]).max() < 1e-6
    assert min(np.abs(r - 0.8).min(), np.abs(r - 1.2).min()) > 0.099
    d = rows["value"].astype(np.float64) - rows["v_old"]
    assert np.abs(np.abs(d) - 0.2).min() > 0.099 and (d == 0).any()
    v_c = rows["v_old"] + np.clip(d, -0.2, 0.2)
    gap = np.abs((rows["value"] - rows["ret"].astype(np.float64)) ** 2 - (v_c - rows["ret"]) ** 2)
    assert gap[np.abs(d) > 0.2].min() > 0.05
    assert (rows["adv"] > 0).any() and (rows["adv"] < 0).any() and np.abs(rows["adv"]).min() >= 0.2


@pytest.mark.parametrize("entropy_bonus", [False, True])
@pytest.mark.parametrize("B", [1, 5, 64, 65, 257])
def test_oracle_equals_autograd_on_the_update_expression(B, entropy_bonus):
    """float64 torch on the CPU, the expression of ppo_update with policy.masked_categorical, against the
    closed forms: 1e-14 absolute on B * gradient and on the statistics."""
    import torch
    from splendor_gym.policy import masked_categorical
    case = make_case(3, 70, 10 + B)
    idx = case_idx(210, B, B)
    rows = case_rows(case, idx)
    sign = -1.0 if entropy_bonus else 1.0
    want = loss_oracle(**{**rows, "ent_coef": sign * COEF["ent_coef"]})
    assert want["bad"] == 0
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    logits, value = t64(rows["logits"]).requires_grad_(), t64(rows["value"]).view(B, 1).requires_grad_()
    mask = t64((rows["mask_bits"][:, None] >> np.arange(NA)) & 1)
    mb = {"logprob": t64(rows["lp_old"]), "value": t64(rows["v_old"]), "adv": t64(rows["adv"]), "ret": t64(rows["ret"])}
    clip_coef, vclip, vf_coef, ent_coef = (COEF[k] for k in ("clip_coef", "vclip", "vf_coef", "ent_coef"))
    probs = masked_categorical(logits, mask)
    new_logprob, entropy, new_value = probs.log_prob(torch.from_numpy(rows["action"]).long()), probs.entropy().mean(), value
    ratio = (new_logprob - mb["logprob"]).exp()
    clip_adv = torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef) * mb["adv"]
    policy_loss = -torch.min(ratio * mb["adv"], clip_adv).mean()
    v_pred = new_value.squeeze(-1)
    v_clipped = mb["value"] + torch.clamp(v_pred - mb["value"], -vclip, vclip)
    value_loss = 0.5 * torch.max((v_pred - mb["ret"]).pow(2), (v_clipped - mb["ret"]).pow(2)).mean()
    loss = policy_loss + vf_coef * value_loss + sign * ent_coef * entropy
    loss.backward()
    approx_kl = (mb["logprob"] - new_logprob).mean()
    assert np.abs(B * logits.grad.numpy() - B * want["dlogits"]).max() <= 1e-14
    assert np.abs(B * value.grad.numpy().reshape(B) - B * want["dvalue"]).max() <= 1e-14
    got = {"loss": loss, "policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy, "approx_kl": approx_kl}
    for name, x in got.items():
        assert abs(float(x.detach()) - want[name]) <= 1e-14, name
    assert want["clipfrac"] == float(((ratio - 1).abs() > clip_coef).double().mean())
    illegal = (mask < 0.5) & (mask.sum(dim=1, keepdim=True) > 0)
    assert (want["dlogits"][illegal.numpy()] == 0).all()


def test_oracle_one_row_by_hand():
    """Two legal actions (0 and 1) with equal logits: p = 1/2 each, lp = -ln 2, H = ln 2, and with
    logprob = -ln 2 the ratio is exactly 1.  A = 2, c = 1/4:
      policy = -min(2, 2) = -2;  g_lp = -A r / B = -2
      dlogits[0] = -2 (1 - 1/2) = -1, dlogits[1] = -2 (0 - 1/2) = +1; the entropy part p (log p + H) is 0
    v = 1, v_old = 1/2, vclip = 1/4: v_c = 3/4; ret = 0: (v-ret)^2 = 1 > (v_c-ret)^2 = 9/16
      value = 1/2, (w1, w2) = (1, 0), dvalue = vf_coef (v - ret) = 1/2
    loss = -2 + 1/2 * 1/2 + 1/4 ln 2; approx_kl = 0; clipfrac = 0."""
    logits = np.zeros((1, NA))
    logits[0, 2:] = 5.0  # illegal columns do not matter
    o = loss_oracle(logits, [1.0], [0b11], [0], [math.log(0.5)], [0.5], [2.0], [0.0], 0.25, 0.25, 0.5, 0.25)
    want = np.zeros(NA)
    want[:2] = (-1.0, 1.0)
    assert np.abs(o["dlogits"][0] - want).max() <= 1e-15 and (o["dlogits"][0, 2:] == 0).all()
    assert o["dvalue"].tolist() == [0.5]
    assert o["policy_loss"] == -2.0 and o["value_loss"] == 0.5 and abs(o["entropy"] - math.log(2.0)) <= 1e-15
    assert abs(o["loss"] - (-1.75 + 0.25 * math.log(2.0))) <= 1e-15
    assert o["approx_kl"] == 0.0 and o["clipfrac"] == 0.0 and o["bad"] == 0
    # the recorded action outside the mask: a bad row, nothing but the count
    o = loss_oracle(logits, [1.0], [0b11], [2], [math.log(0.5)], [0.5], [2.0], [0.0], 0.25, 0.25, 0.5, 0.25)
    assert o["bad"] == 1 and not o["dlogits"].any() and not o["dvalue"].any() and o["loss"] == 0.0


# --------------------------------------------------------------------------------------------
P = 0x10000  # a plausible, aligned, never-dereferenced device address: every case below is refused first
PTRS = ("idx", "mask_bits", "action", "logprob", "value", "adv", "ret", "stats", "logits", "new_value", "dlogits",
        "dvalue", "out", "errors", "scratch")


def _lib():
    from splendor_gym import _native
    return _native, _native.load_library()  # dlopen only: no GPU needed


def _refused(lib, code, word):
    assert code < 0, code
    msg = lib.spl_last_error()
    assert msg and word.encode() in msg, msg


def test_struct_sizes_and_scratch_bytes():
    native, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splendor_ppo.h")).read()
    assert re.search(r"#define SPL_PPO_ABI 1\b", src) and lib.spl_abi_version() == 9
    body = lambda name: re.search(r"typedef struct \{([^}]*)\} " + name + ";", src).group(1)
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = lambda text: [n.strip(" *") for decl in strip(text).split(";") if decl.strip()
                          for n in decl.strip().split(None, 2 if decl.strip().startswith("const") else 1)[-1].split(",")]
    assert names(body("spl_ppo_loss_out_t")) == [f[0] for f in native.PpoLossOut._fields_]
    assert names(body("spl_ppo_loss_t")) == [f[0] for f in native.PpoLoss._fields_]
    assert ctypes.sizeof(native.PpoLossOut) == 6 * 8 + 4 + 4
    assert ctypes.sizeof(native.PpoLoss) == 4 * 4 + 10 * 8 + 4 * 4 + 5 * 8
    assert ctypes.sizeof(native.PpoStats) == 48 and ctypes.sizeof(native.PpoGather) == 16 + 17 * 8  # unchanged
    # six float64 partial sums per workgroup of 256 rows
    assert [lib.spl_ppo_loss_scratch_bytes(B) for B in (1, 256, 257, 65536)] == [48, 48, 96, 256 * 48]
    for B in (0, -1):
        assert lib.spl_ppo_loss_scratch_bytes(B) < 0 and b"positive" in lib.spl_last_error()


def test_loss_refusals():
    native, lib = _lib()
    full = dict(K=4, T=4, normalize=1, reserved=0, clip_coef=0.2, vclip=0.2, vf_coef=0.5, ent_coef=0.03, **{k: P for k in PTRS})
    arg = lambda **kw: ctypes.byref(native.PpoLoss(**kw))
    _refused(lib, lib.spl_ppo_loss(4, None, None), "null")
    for B in (0, -1):
        _refused(lib, lib.spl_ppo_loss(B, arg(**full), None), "positive")
    for name in ("K", "T"):
        for bad in (0, -2):
            _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, name: bad}), None), "positive")
    for name in PTRS:
        _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, name: None}), None), "null")
    for name in ("idx", "mask_bits", "stats", "out", "errors", "scratch"):
        _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, name: P + 4}), None), "aligned")
    _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, "normalize": 0, "stats": P + 4}), None), "aligned")
    for name in ("logprob", "value", "adv", "ret", "logits", "new_value", "dlogits", "dvalue"):
        for off in (1, 2, 3):
            _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, name: P + off}), None), "aligned")
    for name in ("clip_coef", "vclip", "vf_coef", "ent_coef"):
        _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, name: float("nan")}), None), "NaN")
    for name in ("clip_coef", "vclip", "vf_coef"):
        _refused(lib, lib.spl_ppo_loss(4, arg(**{**full, name: -0.125}), None), "negative")
