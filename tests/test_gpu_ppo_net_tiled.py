"""The tiled PPO network passes on the device (spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled,
DeviceNets(tiled=...)): the same BYTES as spl_ppo_net_forward / spl_ppo_net_backward, which test_gpu_ppo_net.py
holds against the float64 oracle.  The f32-input matrix instruction is a k-ordered chain of fused multiply-adds,
and so are the existing kernels, so every comparison here is on int32 views and none has a tolerance: a
difference is a bug in the tile's summation order, padding or epilogue."""
import copy
import re

import numpy as np
import pytest

from test_gpu_ppo_adam import EPS, LR, bits, run_cli, run_update
from test_gpu_ppo_loss import DEV, collected  # noqa: F401  (collected: a module fixture)
from test_gpu_ppo_net import (COEF, CRAFTED, P, SENTINEL, agents, gaps_untouched, gradients, in_arena, make_idx,  # noqa: F401
                              minibatch, store)
from test_ppo_net_host import NA, NETS, tensors_of

pytestmark = pytest.mark.gpu

H = 256
OUTPUTS = ("logits", "value", "act", "scratch", "arena")


def tile_rows():
    from splendor_gym import _native
    return _native.PPO_NET_TILE_ROWS


def passes(agent, store, idx, dlogits, dvalue, *, fill=SENTINEL, backward_tiled=None, floats=False, **nets_kw):
    """DeviceNets(agent, **nets_kw).forward and backward with every output pre-filled with `fill`; `backward_tiled`
    sets nets.tiled between the two calls.  Returns the int32 views of logits, value, the whole of act, the whole
    of scratch and the gradients' arena, by how much store.errors rose in each of the two calls, and with
    `floats` the float32 host copies under "f"."""
    import torch
    from splendor_gym.ppo import DeviceNets
    a, arena, views = in_arena(agent)
    arena.fill_(fill)
    nets = DeviceNets(a, **nets_kw)
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(tensors_of(a), views))  # taken in place
    B = len(idx)
    bufs = nets._buffers(B)
    for name in ("logits", "value", "act", "scratch"):
        bufs[name].fill_(fill)
    d_idx = torch.from_numpy(idx).to(DEV)
    e0 = int(store.errors.item())
    logits, value = nets.forward(store, d_idx)
    e1 = int(store.errors.item())
    if backward_tiled is not None:
        nets.tiled = backward_tiled  # the buffers are per B and shared between the two paths
    nets.backward(store, d_idx, torch.from_numpy(dlogits).to(DEV), torch.from_numpy(dvalue).to(DEV))
    torch.cuda.synchronize()
    e2 = int(store.errors.item())
    if fill == SENTINEL:
        assert gaps_untouched(arena, views)
    dev = {"logits": logits, "value": value, "act": bufs["act"], "scratch": bufs["scratch"], "arena": arena}
    out = {k: v.reshape(-1).view(torch.int32).clone() for k, v in dev.items()}
    out["views"] = [v.reshape(-1).view(torch.int32).clone() for v in views]
    out["errors"] = (e1 - e0, e2 - e1)
    if floats:
        out["f"] = {"logits": logits.cpu().numpy().copy(), "value": value.cpu().numpy().copy(),
                    "act": bufs["act"].cpu().numpy()[:4 * B * H].reshape(2, 2, B, H).copy(),
                    "dz": bufs["scratch"].cpu().numpy()[:4 * B * H].reshape(2, 2, B, H).copy(),
                    "grads": {net: [v.cpu().numpy().copy() for v in views[6 * i:6 * i + 6]] for i, net in enumerate(NETS)}}
    return out


def same_bytes(label, got, want):
    import torch
    for name in OUTPUTS:
        differ = int((got[name] != want[name]).sum())
        print(f"{label} {name}: {differ} of {got[name].numel()} words differ")
    for name in OUTPUTS:
        assert torch.equal(got[name], want[name]), (label, name)
    assert got["errors"] == want["errors"], label


def every_word_written(out, B):
    """logits, value, act, the dZ head of scratch and the twelve gradients hold no word of the fill."""
    import torch
    fill = int(torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item())
    assert out["logits"].numel() == B * NA and out["value"].numel() == B and out["act"].numel() == 4 * B * H
    for name, words in (("logits", out["logits"]), ("value", out["value"]), ("act", out["act"]),
                        ("dZ", out["scratch"][:4 * B * H])):
        assert not bool((words == fill).any()), name
    assert len(out["views"]) == 12 and not any(bool((v == fill).any()) for v in out["views"])


def batch_sizes():
    R = tile_rows()
    return sorted({1, R - 1, R, R + 1, 2 * R + 1, 7, 8, 9, 129, 257, 4097, 4225})


_existing = {}


def existing(agents, store, kind, B):
    """The existing path's bytes for make_idx(B, B) and gradients(B, B): computed once, shared, never changed."""
    if (kind, B) not in _existing:
        idx = make_idx(B, B)
        _existing[kind, B] = passes(agents[kind], store, idx, *gradients(B, B), tiled=False)
    return _existing[kind, B]


@pytest.mark.parametrize("kind", ["trained", "fresh"])
@pytest.mark.parametrize("B", batch_sizes())
def test_same_bytes_as_the_existing_path(store, agents, kind, B):
    """One row; one short of, exactly, one past a row tile and one past two; the existing path's edges (its
    forward tile of 8, one and two chunks of the sums over rows); 4 097 rows (33 chunks: partial 0 sums a second
    chunk, of one row) and 4 225 (34 chunks: partial 0 a whole second chunk, partial 1 a ragged one).  Every
    word of every output is written; the gaps between the gradients are not."""
    want = existing(agents, store, kind, B)
    got = passes(agents[kind], store, make_idx(B, B), *gradients(B, B), tiled=True)
    every_word_written(want, B)
    every_word_written(got, B)
    same_bytes(f"tiled {kind} B={B}", got, want)
    assert got["errors"] == (0, 0)


def test_either_forward_goes_with_either_backward(store, agents):
    B = tile_rows() + 1
    want = existing(agents, store, "trained", B)
    idx, (dlogits, dvalue) = make_idx(B, B), gradients(B, B)
    for forward_tiled, backward_tiled in ((True, False), (False, True)):
        got = passes(agents["trained"], store, idx, dlogits, dvalue, tiled=forward_tiled, backward_tiled=backward_tiled)
        every_word_written(got, B)
        same_bytes(f"forward tiled={forward_tiled} backward tiled={backward_tiled}", got, want)


def test_column_295_and_bad_rows(store, agents):
    """The crafted positions (a move count of 256 or more, so column 295 takes its second byte) and the three bad
    positions -1, K * T and 2^40, one the last row of a row tile, one the first row of the next and one the
    batch's last: the existing path's bytes, exact zeros, and store.errors up by 3 in the forward call alone."""
    import torch
    R = tile_rows()
    B = 2 * R + 1
    idx = make_idx(B, 17)
    assert set(CRAFTED) <= set(idx[:5].tolist())
    assert (store.obs_u8.view(P, 300)[list(CRAFTED), 297] > 0).all()
    idx[[R - 1, R, 2 * R]] = (-1, P, 2 ** 40)
    dlogits, dvalue = gradients(17, B)
    planes = store.obs_u8.clone()
    want = passes(agents["trained"], store, idx, dlogits, dvalue, tiled=False)
    got = passes(agents["trained"], store, idx, dlogits, dvalue, tiled=True)
    same_bytes("bad rows", got, want)
    assert got["errors"] == (3, 0)
    logits, value = got["logits"].view(B, NA), got["value"]
    for r in (R - 1, R, 2 * R):
        assert not bool(logits[r].any()) and int(value[r]) == 0  # +0.0 in every word
    assert bool(logits[R - 2].any()) and bool(logits[R + 1].any())
    assert bool((store.obs_u8 == planes).all())
    # the second byte counts: without it the crafted rows' logits differ
    from splendor_gym.ppo import DeviceNets, PPORolloutStore
    cleared = PPORolloutStore(store.num_steps, store.num_envs, DEV)
    cleared.obs_u8.copy_(store.obs_u8)
    cleared.obs_u8[:, :, 297] = 0
    low, _ = DeviceNets(copy.deepcopy(agents["trained"]), tiled=True).forward(cleared, torch.from_numpy(idx).to(DEV))
    low = low.view(torch.int32)
    crafted = [r for r in range(B) if idx[r] in CRAFTED]
    plain = [r for r in range(B) if 0 <= idx[r] < P and idx[r] not in CRAFTED]
    assert len(crafted) >= 5 and len(plain) >= B - 16
    assert all(not torch.equal(low[r], logits[r]) for r in crafted) and all(torch.equal(low[r], logits[r]) for r in plain)


def test_overwrite_and_determinism(store, agents):
    import torch
    B = 257
    idx = make_idx(B, 4)
    idx[10] = -1
    dlogits, dvalue = gradients(4, B)
    first = passes(agents["fresh"], store, idx, dlogits, dvalue, tiled=True)
    dirty = passes(agents["fresh"], store, idx, dlogits, dvalue, tiled=True, fill=123.0)
    for name in ("logits", "value", "act"):
        assert torch.equal(first[name], dirty[name]), name
    assert torch.equal(first["scratch"][:4 * B * H], dirty["scratch"][:4 * B * H])
    assert all(torch.equal(x, y) for x, y in zip(first["views"], dirty["views"]))
    # and a second backward on top of the first call's gradients
    from splendor_gym.ppo import DeviceNets
    a, arena, views = in_arena(agents["fresh"])
    nets = DeviceNets(a, tiled=True)
    d = lambda x: torch.from_numpy(x).to(DEV)
    nets.forward(store, d(idx))
    nets.backward(store, d(idx), d(dlogits), d(dvalue))
    once = arena.view(torch.int32).clone()
    nets.backward(store, d(idx), d(dlogits), d(dvalue))
    assert torch.equal(arena.view(torch.int32), once) and torch.equal(once, first["arena"])


def test_one_tiled_minibatch_is_one_linear_graph(collected):
    """test_gpu_ppo_net.py's test_one_minibatch_is_one_linear_graph with the tiled calls: forward, loss, backward
    and DeviceAdam.step captured after an eager first run, replayed twice with set_lr between: bit-equal to the
    same three minibatches eager, on the tiled calls and on the existing ones."""
    import torch
    from splendor_gym.ppo import DeviceAdam, DeviceNets
    agent, store = collected
    idx = torch.arange(64, 192, dtype=torch.int64, device=DEV)
    rates = (LR, LR, 1e-3)

    def make(tiled):
        a = copy.deepcopy(agent)
        return a, DeviceNets(a, tiled=tiled), DeviceAdam(list(a.parameters()), lr=LR, eps=EPS)

    eager = {}
    for tiled in (False, True):
        a_e, nets_e, opt_e = make(tiled)
        for k, lr in enumerate(rates):
            if k == 2:
                opt_e.set_lr(lr)
            minibatch(nets_e, store, opt_e, idx)
        eager[tiled] = (bits(a_e.parameters()) + bits([opt_e._exp_avg, opt_e._exp_avg_sq]), opt_e.read_state(),
                        opt_e._state.view(torch.int64).clone())
    a_g, nets_g, opt_g = make(True)
    minibatch(nets_g, store, opt_g, idx)  # eager: loads every kernel, sizes every buffer
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    streams = set()
    with torch.cuda.graph(graph):
        capture = torch.cuda.current_stream().cuda_stream
        minibatch(nets_g, store, opt_g, idx)
        streams.update((nets_g._stream().value, store._stream().value, opt_g._stream().value,
                        torch.cuda.current_stream().cuda_stream))
    assert streams == {capture}  # one stream from the first call to the last: no branch to join
    assert opt_g.read_state()["step"] == 1  # capturing ran nothing
    graph.replay()
    opt_g.set_lr(rates[2])
    graph.replay()
    torch.cuda.synchronize()
    got = bits(a_g.parameters()) + bits([opt_g._exp_avg, opt_g._exp_avg_sq])
    for tiled in (True, False):
        want, state, raw = eager[tiled]
        assert opt_g.read_state() == state and state["step"] == 3 and state["lr"] == rates[2]
        assert torch.equal(opt_g._state.view(torch.int64), raw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), tiled
    assert not torch.equal(bits(a_g.parameters())[0], bits(agent.parameters())[0])  # and the steps were taken


@pytest.mark.parametrize("device_adam", [True, False])
def test_ppo_update_with_tiled_nets(collected, device_adam):
    import torch
    agent, store = collected
    (p_ref, res_ref, _), (p, res, _) = (run_update(agent, store, device_adam, 0.0, tiled=tiled) for tiled in (False, True))
    p_ref, p = bits(p_ref), bits(p)
    assert res_ref["optimizer_steps"] == 8 and set(res) == set(res_ref)
    assert all(torch.equal(x, y) for x, y in zip(p, p_ref))
    assert not torch.equal(p[0], bits(agent.parameters())[0])
    for name in res_ref:
        a, b = np.float64(res[name]), np.float64(res_ref[name])
        assert a.tobytes() == b.tobytes(), (name, res[name], res_ref[name])
    assert int(store.errors.item()) == 0


class Counting:
    """The library with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_auto_switches_at_tiled_min_rows(store, agents):
    import torch
    from splendor_gym.ppo import DeviceNets
    nets = DeviceNets(copy.deepcopy(agents["fresh"]), tiled="auto")
    nets.lib = lib = Counting(nets.lib)
    edge = DeviceNets.TILED_MIN_ROWS
    assert 1 < edge <= DeviceNets.MAX_ROWS
    for B, suffix in ((edge - 1, ""), (edge, "_tiled"), (edge + 1, "_tiled"), (1, "")):
        lib.calls.clear()
        idx = torch.from_numpy(make_idx(B, 1)).to(DEV)
        nets.forward(store, idx)
        nets.backward(store, idx, torch.zeros(B, NA, device=DEV), torch.zeros(B, device=DEV))
        passes_called = {k: v for k, v in lib.calls.items() if k.endswith(("forward", "backward", "_tiled"))}
        assert passes_called == {"spl_ppo_net_forward" + suffix: 1, "spl_ppo_net_backward" + suffix: 1}, B
    torch.cuda.synchronize()


def test_cli_tiled_nets():
    """python -m splendor_gym.scripts.ppo_device --device-adam --tiled-nets on at the smallest shape prints the
    update lines of the same run with --device-nets, apart from sps."""
    first, second = ([re.sub(r" sps \d+", "", ln) for ln in run_cli("--update-epochs", "1", "--device-adam", *switch, updates=2)]
                     for switch in (("--device-nets",), ("--tiled-nets", "on")))
    assert " sps " not in first[0], first
    assert first == second
