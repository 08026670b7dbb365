"""What the bf16 PPO network passes (spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16, include/splendor_ppo.h)
compute, in numpy: round-to-nearest-even to bf16, float64 products of rounded operands with their error bound,
the split of input column 295, and an emulator of both passes (float64 sums of rounded operands) that measures
what bf16 operands cost by construction.  No torch, no device."""
import numpy as np

NETS = ("actor", "critic")
IN, H, NA = 297, 256, 45
HI_POS = 297  # the pad position of k that carries 256 * byte 297, against W1[:, 295]
U = 2.0 ** -23  # twice float32's unit round-off: covers a truncating adder inside the matrix instruction


def to_bf16(x):
    """float32 values rounded to bf16, round-to-nearest-even, returned as float32 (low 16 bits zero).  Integer
    arithmetic on the uint32 view: add 0x7fff plus the bit that will be the last kept, drop the low half.  NaNs
    and infinities are not handled (no test has one)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = x.view(np.uint32).astype(np.uint64)
    w = (w + 0x7FFF + ((w >> 16) & 1)) & 0xFFFF0000
    return w.astype(np.uint32).view(np.float32).reshape(x.shape)


def split_inputs(rows):
    """uint8 [B, 300] compact rows -> float64 [B, 298]: the 297 bytes as they are (column 295 its low byte
    alone) and, as position 297, 256 * byte 297.  Every value is exact in bf16."""
    rows = np.asarray(rows)
    x = np.zeros((len(rows), IN + 1))
    x[:, :IN] = rows[:, :IN]
    x[:, HI_POS] = 256.0 * rows[:, 297]
    return x


def split_weights(w1):
    """[256, 297] -> [256, 298]: column 295 once more as position 297."""
    return np.concatenate([np.asarray(w1, dtype=np.float64), np.asarray(w1, dtype=np.float64)[:, 295:296]], axis=1)


def fold_columns(dw1):
    """[256, 298] sums over rows -> [256, 297]: position 297 added into column 295."""
    out = dw1[:, :IN].copy()
    out[:, 295] += dw1[:, HI_POS]
    return out


def gamma(n):
    return n * U / (1.0 - n * U)


def product(a, b, start=None, n_extra=0):
    """(a @ b [+ start], bound) in float64: every product a[i, k] b[k, j] is taken as exact, so the only error of
    a float32 evaluation is that of its n float32 additions in some order, n = the k terms + the start value +
    n_extra (the combination of partial sums): bound = gamma_n * (|a| @ |b| [+ |start|]), gamma_n = n U / (1 - n U)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    y, mag = a @ b, np.abs(a) @ np.abs(b)
    n = a.shape[1] + n_extra
    if start is not None:
        y, mag, n = y + start, mag + np.abs(start), n + 1
    return y, gamma(n) * mag


def ulp32(x):
    """the float32 unit in the last place at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def emulate(params, rows, dlogits, dvalue, bad=None):
    """Both passes as the contract states them, with float64 sums: matrix products of operands rounded by to_bf16
    (the inputs exact), the saved planes H1, H2, dZ2, dZ1 rounded to float32 as stored, the critic's output unit,
    its dZ2 and the bias gradients from unrounded operands.  params: {"actor": [w1, b1, w2, b2, w3, b3], "critic":
    [...]} float32 or float64 arrays of float32 values; rows uint8 [B, 300].  Returns test_ppo_net_host.net_oracle's
    layout: logits [B, 45], value [B], grads {net: [dW1, db1, dW2, db2, dW3, db3]}."""
    B = len(rows)
    bad = np.zeros(B, dtype=bool) if bad is None else np.asarray(bad, dtype=bool)
    x = split_inputs(rows)
    x[bad] = 0.0
    bf = lambda v: to_bf16(np.asarray(v, dtype=np.float32)).astype(np.float64)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    out = {"grads": {}}
    for net, d_out in (("actor", np.asarray(dlogits, dtype=np.float64).reshape(B, NA)),
                       ("critic", np.asarray(dvalue, dtype=np.float64).reshape(B, 1))):
        w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float64) for p in params[net])
        h1 = f32(np.tanh(x @ split_weights(bf(w1)).T + b1))
        h2 = f32(np.tanh(bf(h1) @ bf(w2).T + b2))
        d = d_out.copy()
        d[bad] = 0.0
        if net == "actor":
            y = bf(h2) @ bf(w3).T + b3
            dz2 = f32((bf(d) @ bf(w3)) * (1.0 - h2 * h2))
        else:
            y = h2 @ w3.T + b3
            dz2 = f32((d @ w3) * (1.0 - h2 * h2))
        y[bad] = 0.0
        dz1 = f32((bf(dz2) @ bf(w2)) * (1.0 - h1 * h1))
        out["grads"][net] = [fold_columns(bf(dz1).T @ x), dz1.sum(0), bf(dz2).T @ bf(h1), dz2.sum(0),
                             bf(d).T @ bf(h2), d.sum(0)]
        out["logits" if net == "actor" else "value"] = y if net == "actor" else y[:, 0]
    return out


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))
