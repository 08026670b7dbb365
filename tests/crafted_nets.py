"""Crafted ActorCritic networks, observations and logit tables for the policy kernels (spl_policy.hip,
spl_policy32.hip) and the PPO network passes (spl_ppo_net.hip, spl_ppo_net_tiled.hip), each with a numpy float64
evaluation of the same module.  A plain helper: no test, no fixture, nothing here needs a GPU.

What the networks are for (the kernels' own comments promise all of it, default-initialised and trained weights
on engine observations reach none of it):
  * probe networks: the kernel's tanh of a CHOSEN argument arrives in an output with no other rounding;
  * range networks: weight rows scaled by powers of two, outliers inside a row, all-zero rows;
  * observation sweeps: one value above 255 in every column, in one table of a wave and in all of them;
  * logit tables: W3 = 0 and b3 = a chosen row, so every table's logits are exactly that row.
Everything is seeded and built on the CPU, so the CPU tests (test_policy_crafted_host.py) judge exactly the
inputs the GPU tests run."""
import os

import numpy as np

from test_ppo_net_host import H, IN, NA, NETS, ROW, params_of

GROUPS = ((0, 12), (12, 24), (24, 36), (36, 45))  # act_epilogue4: lane group g takes actions 12g .. 12g + 11
BRANCH = np.float32(0.625)                        # tanh_acc: the polynomial below, exp2 / rcp from here up
SATURATED = 20.0  # 2 / (exp(40) + 1) = 8.5e-18 < 2^-25: any fp32 evaluation of 1 - 2 / (e + 1) gives exactly 1


def _next(x, n):
    """The float32 n steps above (n > 0) or below (n < 0) x."""
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf))
    return x


def tanh_one():
    """The smallest float32 whose float64 tanh rounds to 1.0f (~9.01)."""
    lo, hi = np.float32(8.0).view(np.int32), np.float32(10.0).view(np.int32)
    while hi - lo > 1:
        mid = np.int32((int(lo) + int(hi)) // 2)
        if np.float32(np.tanh(np.float64(mid.view(np.float32)))) == np.float32(1.0):
            hi = mid
        else:
            lo = mid
    return hi.view(np.float32)


def special_magnitudes():
    """The chosen arguments (float32, positive; zero first)."""
    t1 = tanh_one()
    vals = [0.0, 2.0 ** -126, 1e-30, 1e-8, 1e-4, 1e-2]
    vals += [_next(BRANCH, k) for k in (-3, -2, -1, 0, 1, 2, 3)]
    vals += [0.7, 1.0, 2.0, 5.0]
    vals += [_next(t1, k) for k in (-2, -1, 0, 1, 2)]
    vals += [20.0, 44.0, 45.0, 88.0, 100.0, 1e4, 3e38]
    return np.array(vals, dtype=np.float32)


def sweep(seed=0):
    """float32 [256]: every special magnitude with both signs, the rest log-uniform in [1e-6, 30] with random
    signs, in a seeded random order (so the special values fall on every tile and register position)."""
    rng = np.random.default_rng(seed)
    m = special_magnitudes()
    vals = np.concatenate([m, -m[1:]])
    rest = H - len(vals)
    fill = np.exp(rng.uniform(np.log(1e-6), np.log(30.0), size=rest)) * rng.choice([-1.0, 1.0], size=rest)
    out = np.concatenate([vals, fill]).astype(np.float32)[rng.permutation(H)]
    assert np.isfinite(out).all() and ((out == 0) | (np.abs(out) >= np.float32(2.0 ** -126))).all()
    return out


# ---- the float64 evaluation -----------------------------------------------------------------------------
def forward64(params, x, tanh=np.tanh):
    """Both networks in float64 on x [n, 297].  params: params_of's layout (or any arrays of that layout).
    Per network: pre-activations z1, z2, activations h1, h2, the output y [n, out] and mag = sum_k |w3_k h2_k|
    + |b3| per output (the scale of a layer-3 row's rounding)."""
    x = np.asarray(x, dtype=np.float64)
    out = {}
    for net in NETS:
        w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float64) for p in params[net])
        z1 = x @ w1.T + b1
        h1 = tanh(z1)
        z2 = h1 @ w2.T + b2
        h2 = tanh(z2)
        out[net] = {"z1": z1, "h1": h1, "z2": z2, "h2": h2, "y": h2 @ w3.T + b3,
                    "mag": np.abs(h2) @ np.abs(w3).T + np.abs(b3)}
    return out


def outputs64(agent_or_params, x, **kw):
    """(logits [n, 45], value [n]) of forward64."""
    p = agent_or_params if isinstance(agent_or_params, dict) else params_of(agent_or_params)
    r = forward64(p, x, **kw)
    return r["actor"]["y"], r["critic"]["y"][:, 0]


def new_agent(seed):
    import torch
    from splendor_gym.policy import ActorCritic
    torch.manual_seed(seed)
    return ActorCritic().eval()


def set_params(agent, params):
    """Write params (params_of's layout) into the module as float32; returns the agent."""
    import torch
    with torch.no_grad():
        for net in NETS:
            seq = getattr(agent, net)
            for j, i in enumerate((0, 2, 4)):
                seq[i].weight.copy_(torch.from_numpy(np.asarray(params[net][2 * j], dtype=np.float32)))
                seq[i].bias.copy_(torch.from_numpy(np.asarray(params[net][2 * j + 1], dtype=np.float32)))
    return agent


# ---- observations -----------------------------------------------------------------------------------------
def real_rows(n, first=0):
    """int32 [n, 297]: engine observations of the committed 2-player trajectories (tests/golden/traj_p2.npz,
    plies 8 .. 47 of its 16 recorded games)."""
    full = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_p2.npz"))["full_obs"]
    rows = full[:, 8:48].transpose(1, 0, 2).reshape(-1, IN).astype(np.int32)
    assert first + n <= len(rows)
    return rows[first:first + n].copy()


def compact(obs):
    """uint8 [n, 300] rows of int32 observations with values in [0, 255] but column 295 in [0, 65535]."""
    obs = np.asarray(obs)
    c = np.delete(obs, 295, axis=1)
    assert obs.min() >= 0 and c.max() <= 255 and obs[:, 295].max() <= 65535
    rows = np.zeros((len(obs), ROW), dtype=np.uint8)
    rows[:, :IN] = obs & 0xFF
    rows[:, 297] = obs[:, 295] >> 8
    return rows


def expand(rows):
    """int32 [n, 297] of compact rows (column 295 = byte 295 + 256 * byte 297)."""
    x = rows[:, :IN].astype(np.int32)
    x[:, 295] += 256 * rows[:, 297].astype(np.int32)
    return x


EXACT_VALUES = (257, 383, 32769, 333, 65407)  # 256 + odd, 383, ...: x - bf16(x) = 1, -1, 1, 1, 127, never 0
F16_VALUES = (1025, 2047)                     # the fp16-plane format: exact below 2048
SWEEP_N, SWEEP_LAUNCHES = 145, 3
SWEEP_BOOST = 2.0
_SINGLE = tuple(range(0, 112)) + tuple(range(128, 145))  # rows of a launch that carry ONE large value
_ALL = tuple(range(112, 128))                            # wave 7 of a launch: every table carries large values


def sweep_magnitude(fmt, c):
    """The magnitude every large value of column c has."""
    vals = EXACT_VALUES if fmt == "fp32" else F16_VALUES
    return vals[c % len(vals)]


def obs_sweep(fmt):
    """Three launches of 145 int32 rows (fmt "fp32": the exact format's values, "fp32_f16x2": the fp16 planes').
    In each launch waves 0-6 and the ragged second workgroup (rows 128-144) hold rows with ONE large value, in
    consecutive columns, so a wave has each of its columns large in exactly one table; wave 7 (rows 112-127) has
    every table large in every third column (column % 3 == launch).  Over the three launches the 387 single rows
    visit every column, and the three wave-7s cover every column in all 16 tables.  A column's large values all
    have one magnitude (sweep_magnitude) and both signs.  Returns (obs int32 [3, 145, 297], column [3, 145] of
    the single rows' large value or -1)."""
    obs = real_rows(SWEEP_N * SWEEP_LAUNCHES).reshape(SWEEP_LAUNCHES, SWEEP_N, IN)
    col = np.full((SWEEP_LAUNCHES, SWEEP_N), -1, dtype=np.int64)
    k = 0
    for L in range(SWEEP_LAUNCHES):
        for r in _SINGLE:
            c = k % IN
            obs[L, r, c] = sweep_magnitude(fmt, c) * (1 if (k // 5) % 2 == 0 else -1)
            col[L, r] = c
            k += 1
        for i, r in enumerate(_ALL):
            for c in range(L, IN, 3):
                obs[L, r, c] = sweep_magnitude(fmt, c) * (1 if (i + c // 3) % 2 == 0 else -1)
    return obs, col


def sweep_agent(obs, seed=21):
    """A default-initialised network whose W1 column c is multiplied by SWEEP_BOOST and divided by the largest
    |obs[..., c]| of the batch (by 1 where that is 0), in both networks: a large value contributes to a
    pre-activation what an observation value of 2 did, and the pre-activations stay unsaturated."""
    agent = new_agent(seed)
    p = params_of(agent)
    scale = np.maximum(np.abs(np.asarray(obs).reshape(-1, IN)).max(axis=0), 1).astype(np.float64)
    for net in NETS:
        p[net][0] = p[net][0] * SWEEP_BOOST / scale
    return set_params(agent, p)


def compact_rows(fmt, n=SWEEP_N):
    """uint8 [n, 300] compact rows: all bytes 0; bytes 0..296 all 255 with byte 297 = 0, 1 and the format's
    largest (255: column 295 = 65535 for the exact format and the PPO store; 7: 2047 for the fp16 planes); real
    rows with byte 297 = 0, 1 and that largest; the rest real rows."""
    top = 255 if fmt != "fp32_f16x2" else 7
    rows = compact(real_rows(n, first=40))
    rows[0] = 0
    for i, b in enumerate((0, 1, top)):
        rows[1 + i, :IN] = 255
        rows[1 + i, 297] = b
        rows[4 + i, 297] = b
        rows[n - 1 - i, 297] = b  # and in the ragged last wave
    rows[:, 298:] = 0
    return rows


# ---- probe networks -----------------------------------------------------------------------------------------
PROBE_IMAGES = 6  # 6 x 45 = 270 >= 256 selections: every hidden unit is read by some logit
CRITIC_UNITS = (0, 37, 90, 143, 200, 255)  # tiles 0, 2, 5, 8, 12, 15; registers 0, 1, 2, 3, 0, 3 of groups 0, 1, 2, 3, 2, 3


def critic_values():
    return np.array([_next(BRANCH, -1), BRANCH, -1e-4, 2.0, -tanh_one(), 1e-30], dtype=np.float32)


def probe_units(image):
    return (NA * image + np.arange(NA)) % H


def probe_biases(image):
    """(actor sweep [256], critic sweep [256]): the critic's has its image's chosen value at its selected unit."""
    a = sweep()
    c = a.copy()
    c[CRITIC_UNITS[image]] = critic_values()[image]
    return a, c


def probe_agent(layer, image):
    """layer 2: W1 = 0, b1 = 0, W2 = 0, b2 = sweep, W3 one-hot on probe_units(image), b3 = 0: logit j is the
    kernel's tanh(b2[u_j]).  layer 1: W1 = 0, b1 = sweep, W2 = identity, b2 = 0, the same W3: logit j is
    tanh(tanh(b1[u_j])).  The critic the same with its one-hot w3 on CRITIC_UNITS[image]."""
    assert layer in (1, 2) and 0 <= image < PROBE_IMAGES
    z = np.zeros
    params = {}
    for net, b, units in (("actor", probe_biases(image)[0], probe_units(image)),
                          ("critic", probe_biases(image)[1], np.array([CRITIC_UNITS[image]]))):
        w3 = z((len(units), H))
        w3[np.arange(len(units)), units] = 1.0
        hidden = [z((H, IN)), b, np.eye(H), z(H)] if layer == 1 else [z((H, IN)), z(H), z((H, H)), b]
        params[net] = hidden + [w3, z(len(units))]
    return set_params(new_agent(0), params)


def probe_expected(layer, image):
    """(arguments [46], float64 results [46]): the 45 logits' and then the value's tanh argument and exact result."""
    a, c = probe_biases(image)
    x = np.concatenate([a[probe_units(image)], c[[CRITIC_UNITS[image]]]]).astype(np.float64)
    y = np.tanh(x)
    return x, (np.tanh(y) if layer == 1 else y)


def ulps(got, want64):
    """|got - want| in units of the spacing of the float32 nearest want (float64 arrays)."""
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - want64) / np.spacing(np.abs(w32)).astype(np.float64)


# ---- range networks -----------------------------------------------------------------------------------------
# Rows of layers 1 and 2 are scaled DOWN only (2^-12, 2^-6): a row scaled up as a whole would saturate its tanh on
# integer observations.  What scales up is the consumer's column (x 2^12, x 2^6: the function stays the same, the
# consumer's rows get entries 2^12 apart) and single outliers (x 2^12, x 2^20) on inputs that are exactly zero (the
# unit of an all-zero row), which move a row's largest |w|, and with it the fp16 pack's row exponent, without
# moving the sum.
L1_DOWN = {3: -12, 70: -6, 133: -12, 250: -6}
L1_ZERO = (17, 200)
L2_DOWN = {5: -12, 90: -6, 161: -12, 255: -6}
L2_ZERO = (40, 222)
L2_OUTLIERS = ((8, 17, 12), (100, 200, 20), (5, 17, 20))  # (row, dead input unit, exponent)
L3_FACTORS = (-30, -12, 0, 12, 30)                         # row j of the "out" network: 2^L3_FACTORS[j % 5]
L3_ZERO = (7, 44)
L3_OUTLIERS = {0: 20, 1: 12, 2: 20, 3: 12}                 # row -> exponent of its one outlier (on a live unit)
L3_LOW_BITS = {0: (8, 0x7F), 1: (13, 0x0FFF), 2: (8, 0x7F), 3: (13, 0x0FFF)}  # the outlier's low mantissa bits


def _low_bits(w, count, bits):
    """float32 w with its low `count` mantissa bits replaced.  (8, 0x7F): rounding to 16 significant bits moves it
    by 127/256 of that format's spacing, at least 0.99 x 2^-17 |w|.  (13, 0x0FFF): rounding to 11 bits moves it by
    half of that format's spacing, at least 2^-12 |w|."""
    i = np.asarray(w, dtype=np.float32).view(np.int32)
    return ((i & ~((1 << count) - 1)) | bits).view(np.float32)


def range_agent(kind, obs, seed=31):
    """kind "hidden": the rows of layers 1 and 2 above.  kind "out": layer 3's rows scaled by L3_FACTORS with their
    biases, two all-zero rows, and in rows 0-3 one outlier each on the hidden unit whose |h2| is largest at its
    smallest over `obs` (so that one product dominates the row, with a mantissa whose third bf16 plane is as large
    as it gets); the critic's row x 2^-12.  obs: the int32 batch the network will see."""
    agent = new_agent(seed)
    p = params_of(agent)
    for net in NETS:  # default layer-1 rows reach |z1| ~ 7 on real rows: x 0.4 keeps every pre-activation below 3
        p[net][0] *= 0.4
        p[net][1] *= 0.4
    if kind == "hidden":
        for net in NETS:
            w1, b1, w2, b2, w3, b3 = p[net]
            for r, e in L1_DOWN.items():
                w1[r] *= 2.0 ** e
                b1[r] *= 2.0 ** e
                w2[:, r] *= 2.0 ** -e
            for r in L1_ZERO:
                w1[r] = 0.0
                b1[r] = 0.0
            for r, e in L2_DOWN.items():
                w2[r] *= 2.0 ** e
                b2[r] *= 2.0 ** e
                w3[:, r] *= 2.0 ** -e
            for r in L2_ZERO:
                w2[r] = 0.0
                b2[r] = 0.0
            for r, k, e in L2_OUTLIERS:
                w2[r, k] *= 2.0 ** e
        return set_params(agent, p)
    assert kind == "out"
    h2 = np.abs(forward64(p, obs)["actor"]["h2"]).min(axis=0)
    live = np.argsort(-h2)[:len(L3_OUTLIERS)]
    w3, b3 = p["actor"][4], p["actor"][5]
    for j in range(NA):
        w3[j] *= 2.0 ** L3_FACTORS[j % 5]
        b3[j] *= 2.0 ** L3_FACTORS[j % 5]
    for j in L3_ZERO:
        w3[j] = 0.0
        b3[j] = 0.0
    for (j, e), u in zip(L3_OUTLIERS.items(), live):
        w3[j, u] = np.float64(_low_bits(np.float32(w3[j, u] * 2.0 ** e), *L3_LOW_BITS[j]))
    p["critic"][4] *= 2.0 ** -12
    p["critic"][5] *= 2.0 ** -12
    return set_params(agent, p)


def range_obs(n=SWEEP_N):
    return real_rows(n, first=200)


# ---- logit tables -----------------------------------------------------------------------------------------
PEAKS = (3, 12, 35, 44)  # one action of each lane group (the first of group 1, the last of groups 2 and 3)
TIES = {"tie_11_12": (11, 12), "tie_23_24": (23, 24), "tie_35_36": (35, 36), "tie_0_44": (0, 44), "tie_four": (5, 17, 29, 41)}


def logit_tables():
    """name -> float32 [45]."""
    rng = np.random.default_rng(7)
    base = (np.rint(rng.normal(size=NA) * 32) / 64).astype(np.float32)  # multiples of 1/64: every gap below is exact
    t = {}
    for gap in (20, 90, 200):
        for g, k in enumerate(PEAKS):
            row = base.copy()
            row[k] = np.float32(np.delete(base, k).max() + gap)
            t[f"peak{gap}_group{g}"] = row
    t["equal"] = np.full(NA, 0.5, dtype=np.float32)
    t["equal_plus_1e4"] = np.full(NA, 0.5 + 1e4, dtype=np.float32)
    t["equal_minus_1e4"] = np.full(NA, 0.5 - 1e4, dtype=np.float32)
    for name, members in TIES.items():
        row = np.minimum(base, np.float32(0.75)).copy()
        row[list(members)] = np.float32(1.25)
        t[name] = row
    return t


def frequency_tables():
    """The two rows whose sampling frequencies are checked: all equal, and mildly peaked (gaps <= 3)."""
    rng = np.random.default_rng(8)
    mild = rng.uniform(-1.5, 1.5, size=NA).astype(np.float32)
    return {"equal": np.full(NA, 0.5, dtype=np.float32), "mild": mild}


def masks():
    """name -> int8 [45]."""
    m = {"all": np.ones(NA, dtype=np.int8), "none": np.zeros(NA, dtype=np.int8)}
    for k in (0, 44, 12):
        m[f"only_{k}"] = np.zeros(NA, dtype=np.int8)
        m[f"only_{k}"][k] = 1
    m["last_group"] = np.zeros(NA, dtype=np.int8)
    m["last_group"][36:] = 1
    m["every_other"] = (np.arange(NA) % 2 == 0).astype(np.int8)
    return m


FREQUENCY_MASKS = ("all", "every_other", "last_group")


def logit_agent(row, seed=41):
    """A default-initialised network whose actor has W3 = 0 and b3 = row: every table's logits are exactly `row`
    (a sum of products with zero, then the bias), in all three precisions."""
    agent = new_agent(seed)
    p = params_of(agent)
    p["actor"][4] = np.zeros((NA, H))
    p["actor"][5] = np.asarray(row, dtype=np.float64)
    return set_params(agent, p)


def allowed_set(mask_row):
    """masked_categorical: the legal actions, or every action when none is legal."""
    m = np.asarray(mask_row) != 0
    return m if m.any() else np.ones(NA, dtype=bool)


def log_softmax64(row, allow, subtract_max=True, dtype=np.float64):
    """log-probabilities over `allow` (-inf elsewhere) and the entropy.  dtype float32 and subtract_max False give
    the wrong softmax a kernel without the max would compute."""
    x = np.asarray(row, dtype=dtype)
    with np.errstate(all="ignore"):
        d = x - (x[allow].max() if subtract_max else dtype(0))
        p = np.where(allow, np.exp(d), dtype(0))
        S = p.sum(dtype=dtype)
        logp = np.where(allow, d - np.log(S), -np.inf)
        ent = np.log(S) - (p * np.where(allow, d, 0)).sum(dtype=dtype) / S
    return logp, ent


def first_max(row, mask_row, last=False):
    """logits.masked_fill(mask < 0.5, -inf).argmax(): the first maximum; 0 when nothing is legal.  last: the wrong
    tie rule."""
    m = np.asarray(mask_row) != 0
    if not m.any():
        return 0
    x = np.where(m, np.asarray(row, dtype=np.float64), -np.inf)
    hits = np.flatnonzero(x == x.max())
    return int(hits[-1] if last else hits[0])


def scan_frequencies(row, mask_row, drop_carry=None, ignore_mask_in_carry=False, points=1 << 18):
    """Action frequencies of the inverse-CDF scan of act_epilogue4 over a uniform grid of draws, in float64.  With
    no fault this is the softmax.  drop_carry = g: lane group g's scan starts from 0 instead of the sum of the
    groups before it.  ignore_mask_in_carry: the carries count the groups' disallowed actions too."""
    allow = allowed_set(mask_row)
    x = np.asarray(row, dtype=np.float64)
    p = np.where(allow, np.exp(x - x[allow].max()), 0.0)
    q = np.exp(x - x[allow].max()) if ignore_mask_in_carry else p
    S = p.sum()
    target = (np.arange(points) + 0.5) / points * S
    hit = np.full(points, NA, dtype=np.int64)
    for g, (a, b) in enumerate(GROUPS):
        carry = 0.0 if g == drop_carry else q[:a].sum()
        cum = carry + np.cumsum(p[a:b])
        for j in range(b - a):
            if allow[a + j]:
                here = (cum[j] > target) & (hit > a + j)
                hit[here] = a + j
    last = int(np.flatnonzero(allow)[-1])
    hit[hit == NA] = last
    return np.bincount(hit, minlength=NA) / points


# ---- the tolerances of the GPU comparisons (numpy forms; the CPU tests show that each one can fail) ---------------
PROBE_ULPS = {2: 4.0, 1: 9.0}  # 3.2 ulp derived for tanh_acc with 1-ulp exp2 and rcp, rounded up; twice that plus one rounding
ROW_ULPS = 64 * 2.0 ** -24     # test_gpu_ppo_net.py's factor, here per layer-3 row


def outside(err, tol):
    """Where err is not within tol (a NaN is outside)."""
    return ~(np.asarray(err) <= np.asarray(tol))


def fp32_outside(got, ref, tol=1e-5):
    """test_gpu_policy.fp32_close's rule, per element."""
    return outside(np.abs(got - ref), tol * (np.abs(ref) + 1))


def round_bits(x, bits):
    """x rounded to `bits` significant bits (nearest even), float64."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


def round_row_relative(w, bits):
    """Each row of w rounded to a multiple of 2^-bits of the power of two above the row's largest |w|: one fp16
    plane of the fp16-plane pack (11 bits below the row's exponent)."""
    w = np.asarray(w, dtype=np.float64)
    _, e = np.frexp(np.abs(w).max(axis=-1, keepdims=True))
    q = np.ldexp(1.0, e - bits)
    return np.where(q > 0, np.rint(w / np.where(q > 0, q, 1)) * q, w)
