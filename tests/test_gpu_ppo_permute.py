"""The device permutation and the device-coefficient loss entry on the GPU (spl_ppo_permute, spl_ppo_loss_dev,
splendor_gym.ppo.DevicePermutation, PPORolloutStore.set_loss_coef): every comparison is for equal bytes, against
splendor_gym.ppo.permutation_reference for the permutation and against spl_ppo_loss for the loss head."""
import ctypes

import numpy as np
import pytest

from test_gpu_ppo_loss import DEV, collected  # noqa: F401  (collected: a module fixture)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, -77  # words behind the buffer that must keep their fill
SEEDS = (1234, 2 ** 32 + 77)
DRAWS = (0, 2 ** 32 + 5)
E_ARG, E_RANGE = -1, -3


def word(x):
    x &= 2 ** 64 - 1
    return x - 2 ** 64 if x >= 2 ** 63 else x


def batch_sizes(n):
    """1, an odd value, an even value, n"""
    odd = 341 if n > 341 else 7 if n > 7 else 3
    even = 256 if n > 256 else 6 if n > 6 else 2
    return sorted({b for b in (1, odd, even, n) if b <= n})


def permute(n, B, seed, draw, out=None, state=None, reserved=0):
    """One raw spl_ppo_permute call on fresh buffers: (code, state int64 [2], out int64 [rows * stride + GUARD])."""
    import torch
    from splendor_gym import _native
    lib = _native.load_library()
    stride, rows = (B + 1) // 2 * 2, (n + B - 1) // B
    if state is None:
        state = torch.tensor([word(seed), word(draw)], dtype=torch.int64, device=DEV)
    if out is None:
        out = torch.full((rows * stride + GUARD,), FILL, dtype=torch.int64, device=DEV)
    a = _native.PpoPermute(n=n, B=B, reserved=reserved, state=state.data_ptr(), out=out.data_ptr())
    code = lib.spl_ppo_permute(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, state, out


def padded(ref, B, tail=GUARD):
    """The reference permutation in spl_ppo_permute's layout, the guard band behind it."""
    n = len(ref)
    stride, rows = (B + 1) // 2 * 2, (n + B - 1) // B
    want = np.full(rows * stride + tail, -1, dtype=np.int64)
    want[rows * stride:] = FILL
    i = np.arange(n)
    want[i // B * stride + i % B] = ref
    return want


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1023, 1024, 1025, 2048, 100003])
def test_equals_the_reference(n):
    """Every word the call may write: the permutation at its places, -1 in the pads and the tail, the guard band
    untouched; draw advanced by exactly one, the seed as it was."""
    from splendor_gym.ppo import permutation_reference
    for seed in SEEDS:
        for draw in DRAWS:
            ref = permutation_reference(n, seed, draw)
            for B in batch_sizes(n):
                code, state, out = permute(n, B, seed, draw)
                assert code == 0
                assert np.array_equal(out.cpu().numpy(), padded(ref, B)), (n, B, seed, draw)
                assert state.tolist() == [word(seed), word(draw + 1)], (n, B, seed, draw)


def test_draw_advances_by_one_per_call():
    import torch
    from splendor_gym.ppo import permutation_reference
    n, B, seed = 65, 7, SEEDS[1]
    state = torch.tensor([word(seed), word(2 ** 32 - 2)], dtype=torch.int64, device=DEV)  # across the low word's carry
    for k in range(4):
        code, state, out = permute(n, B, seed, None, state=state)
        assert code == 0 and state.tolist() == [word(seed), 2 ** 32 - 2 + k + 1]
        assert np.array_equal(out.cpu().numpy(), padded(permutation_reference(n, seed, 2 ** 32 - 2 + k), B))


def test_refusals_leave_everything_untouched():
    import torch
    from splendor_gym import _native
    lib = _native.load_library()
    n, B = 100, 7
    state = torch.tensor([5, 9], dtype=torch.int64, device=DEV)
    out = torch.full((15 * 8 + GUARD,), FILL, dtype=torch.int64, device=DEV)
    good = dict(n=n, B=B, reserved=0, state=state.data_ptr(), out=out.data_ptr())
    cases = [("n = 0", dict(n=0), E_RANGE), ("n = 2^31", dict(n=2 ** 31), E_RANGE), ("B = 0", dict(B=0), E_RANGE),
             ("B > n", dict(B=n + 1), E_RANGE), ("reserved", dict(reserved=3), E_ARG), ("null state", dict(state=None), E_ARG),
             ("null out", dict(out=None), E_ARG), ("state misaligned", dict(state=state.data_ptr() + 4), E_ARG),
             ("out misaligned", dict(out=out.data_ptr() + 8), E_ARG)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for label, change, want in cases:
        assert lib.spl_ppo_permute(ctypes.byref(_native.PpoPermute(**{**good, **change})), stream) == want, label
        assert lib.spl_last_error(), label
    torch.cuda.synchronize()
    assert state.tolist() == [5, 9] and bool((out == FILL).all())


def test_device_permutation_object():
    import torch
    from splendor_gym.ppo import DevicePermutation, permutation_reference
    total, B, seed = 1000, 341, SEEDS[1]
    perm = DevicePermutation(total, B, DEV, seed=seed)
    assert (perm.rows, perm.stride, perm.batch_size, perm.total) == (3, 342, 341, 1000) and perm.counter() == 0
    views = perm.minibatches()
    assert [v.numel() for v in views] == [341, 341, 318]
    assert all(v.dtype == torch.int64 and v.is_contiguous() and v.data_ptr() % 16 == 0 for v in views)
    for d in range(2):
        perm.draw()
        assert np.array_equal(torch.cat(perm.minibatches()).cpu().numpy(), permutation_reference(total, seed, d))
        assert [v.data_ptr() for v in perm.minibatches()] == [v.data_ptr() for v in views]  # the same views
    assert perm.counter() == 2 and perm._buf[0, 341].item() == -1 and bool((perm._buf[2, 318:] == -1).all())
    perm.set_counter(2 ** 32 + 5)
    perm.set_seed(SEEDS[0])
    perm.draw()
    assert np.array_equal(torch.cat(perm.minibatches()).cpu().numpy(), permutation_reference(total, SEEDS[0], 2 ** 32 + 5))
    assert perm.counter() == 2 ** 32 + 6
    big = DevicePermutation(10, 64, DEV)  # a batch larger than the store is the whole store
    assert (big.batch_size, big.rows) == (10, 1)
    for bad in ((0, 4), (2 ** 31, 4), (10, 0)):
        with pytest.raises(ValueError):
            DevicePermutation(*bad, DEV)
    with pytest.raises(ValueError):
        DevicePermutation(10, 4, "cpu")


def test_a_captured_draw_follows_the_counter():
    """One draw() captured as a single-stream graph after an eager call, replayed three times: the permutations of
    the next three counter values, which is what three eager calls give."""
    import torch
    from splendor_gym.ppo import DevicePermutation, permutation_reference
    total, B, seed = 1025, 64, 31
    perm = DevicePermutation(total, B, DEV, seed=seed)
    perm.draw()  # eager: loads the kernels
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capture = torch.cuda.current_stream().cuda_stream
        perm.draw()
        assert perm._stream().value == capture
    assert perm.counter() == 1  # capturing ran nothing
    eager = DevicePermutation(total, B, DEV, seed=seed)
    eager.draw()
    for d in (1, 2, 3):
        graph.replay()
        eager.draw()
        got = torch.cat(perm.minibatches())
        assert torch.equal(got, torch.cat(eager.minibatches()))
        assert np.array_equal(got.cpu().numpy(), permutation_reference(total, seed, d))
    assert perm.counter() == eager.counter() == 4


# ---------------------------------------------------------------------------------------------------
COEF = (0.2, 0.2, 0.5, 0.03)


def loss_call(store, idx, logits, value, coef, device_coef):
    """One loss call on sentinel-filled buffers; the bytes of dlogits, dvalue and out."""
    import torch
    bufs = store._loss_buffers(idx.numel())
    bufs["dlogits"].fill_(-77.0)
    bufs["dvalue"].fill_(-77.0)
    bufs["out"].buf.fill_(-77.0)
    store._launch_loss(idx, logits, value, coef, True, device_coef=device_coef)
    torch.cuda.synchronize()
    return [bufs["dlogits"].view(torch.int32).clone(), bufs["dvalue"].view(torch.int32).clone(),
            bufs["out"].buf.view(torch.int64).clone()]


@pytest.mark.parametrize("B", [1, 255, 256, 384])
def test_loss_dev_gives_the_bytes_of_loss(collected, B):
    """One row, a partial last wave, one whole workgroup, two workgroups (duplicates in idx): byte-equal to
    spl_ppo_loss with the block's values as arguments; a rewritten ent_coef is followed; a negative clip_coef
    makes every row bad."""
    import torch
    _, store = collected
    P = store.num_steps * store.num_envs
    g = torch.Generator().manual_seed(B)
    idx = torch.randint(0, P, (B,), generator=g).to(DEV)
    logits, value = torch.randn(B, 45, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
    for coef in (COEF, COEF[:3] + (-0.01,)):  # the second differs in ent_coef alone
        want = loss_call(store, idx, logits, value, coef, False)
        store.set_loss_coef(*coef)
        assert store.loss_coef == coef
        got = loss_call(store, idx, logits, value, (9.0, 9.0, 9.0, 9.0), True)  # the arguments are not looked at
        assert all(torch.equal(a, b) for a, b in zip(got, want)), coef
        assert not bool((got[0] == torch.tensor(-77.0).view(torch.int32).item()).any())
    assert not torch.equal(want[0], loss_call(store, idx, logits, value, COEF, False)[0])  # and ent_coef matters
    before = int(store.errors.item())
    assert int(store._loss_buffers(B)["out"].bad.item()) == 0
    store.set_loss_coef(-0.2, *COEF[1:])
    dlogits, dvalue, _ = loss_call(store, idx, logits, value, COEF, True)
    assert not dlogits.any() and not dvalue.any()
    assert int(store._loss_buffers(B)["out"].bad.item()) == B and int(store.errors.item()) - before == B
    store.errors.zero_()  # the fixture's store as it was
    store.set_loss_coef(*COEF)
