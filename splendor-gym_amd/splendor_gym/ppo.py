"""The PPO rollout store on the device (include/splendor_ppo.h): record, GAE, minibatch gather, and a
collector and update loop on top.

The reference's learner (ppo_splendor.py:287-325) appends per-step numpy copies to Python lists, runs
GAE as a numpy loop on the host and re-uploads everything for the update.  Here the agent's trajectory
stays on the device, step-major [K][T] in the engine's compact formats (uint8 observation rows, 45-bit
masks: 2.8 GB instead of 10.4 GB at 128 steps x 65 536 tables):

  * ``PPORolloutStore``  the planes, ``record_pre`` / ``record_post`` / ``row`` to fill row k around a
    dual step, ``compute_gae`` (ppo_splendor.py:304-314, bit-equal to the numpy loop, and the mean and
    n-1 standard deviation ppo_splendor.py:325 normalises with), ``gather`` (one minibatch expanded
    into ``ActorCritic.get_action_and_value``'s float32 inputs) and ``minibatches``;
  * ``collect``  num_steps iterations of the config-5 loop (FusedActorCritic.act on the env's compact
    rows, DualStepVectorEnv.dual_step), recorded, and the bootstrap value; eager or one hipGraph;
  * ``ppo_update``  the update of ppo_splendor.py:327-361: one loop over ``store.minibatches`` in which a
    loss head leaves every p.grad and the minibatch's statistics, and an optimiser step consumes them.

The head is torch autograd (the default), ``PPORolloutStore.loss`` behind the two networks (``fused_loss``) or
``DeviceNets`` (``device_nets``); the step is a torch.optim optimiser or a ``DeviceAdam``; any head goes with either:

  * ``PPORolloutStore.loss``  everything between the two networks and loss.backward() (masked softmax,
    ratio, clips, means, and their gradients) as one device call on the store's planes (spl_ppo_loss);
  * ``DeviceNets``  the two networks' forward and backward passes as device calls (spl_ppo_net_forward /
    spl_ppo_net_backward) that read the observations from the store by position and write the parameter
    gradients where the optimiser reads them.  ``DeviceNets(agent, tiled=True | "auto")`` runs the passes on
    the LDS-tiled matrix-core kernels built for minibatches of thousands of rows
    (spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled), with the same bytes;
    ``DeviceNets(agent, operands="bf16")`` is the opt-in mixed precision: bf16 operands on the matrix cores,
    float32 accumulation and master weights (spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16), other numbers;
  * ``DeviceAdam``  what follows the head as one device call per minibatch (spl_ppo_adam): the global-norm
    clip, torch.optim.Adam's step and the target-KL early stop, decided on the device, so that
    ``ppo_update`` with it reads the device once per update instead of once per minibatch;
  * ``DevicePermutation``  an epoch's permutation drawn on the device (spl_ppo_permute) from a (seed, draw) block
    that the draw itself advances, laid out so that every minibatch's slice is 16-byte aligned;
    ``permutation_reference`` is the same permutation in numpy, for saying afterwards which positions a
    minibatch held.  With it, a ``DeviceAdam`` and a ``DeviceNets``, ``ppo_update(graph=True)`` captures one
    whole update (every epoch's draw and every minibatch) as one hipGraph and replays it on later calls.

There is no CPU fallback for the store, ``DeviceAdam``, ``DeviceNets`` or ``DevicePermutation``.
"""
import ctypes

import numpy as np

from . import _native
from ._native import NUM_ACTIONS, OBS_DIM, OBS_U8, PpoGae, PpoGather, PpoLoss, PpoLossOut, PpoRecord, check


def _tensor(x, what, dtypes, shape, device=None, or_shape=None):
    """x, if it is a contiguous tensor of one of `dtypes` and of `shape` (None: any; `or_shape`: a second
    one) on `device` (None: anywhere); otherwise a ValueError that names `what`, what it must be and what
    it is."""
    if getattr(x, "dtype", None) in dtypes and (shape is None or x.shape == shape or x.shape == or_shape) and \
            x.is_contiguous() and (device is None or x.device == device):
        return x
    want = f"{dtypes[0]}{'' if shape is None else ' ' + str(list(shape))} tensor{'' if device is None else f' on {device}'}"
    got = f"{x.dtype} {list(x.shape)} on {x.device}{'' if x.is_contiguous() else ' (not contiguous)'}" \
        if hasattr(x, "is_contiguous") else f"a {type(x).__name__}"
    raise ValueError(f"{what} must be a contiguous {want}, not {got}")


def _positions(idx, device):
    """B of the flat positions idx, which must be a non-empty contiguous int64 [B] tensor on `device`."""
    import torch
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous() or \
            idx.device != device or idx.numel() < 1:
        raise ValueError(f"idx must be a non-empty contiguous int64 [B] tensor on {device}")
    return idx.numel()


def _philox4x32_x(c0, c1, c2, c3, k0, k1):
    """The .x word of Philox4x32-10 (csrc/spl_rng.h) for uint64 arrays holding 32-bit words."""
    M32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def permutation_positions(positions, n, seed, draw):
    """Where spl_ppo_permute's permutation of 0 .. n-1 for (seed, draw) sends `positions` (integers in [0, n);
    `draw` may be an array that broadcasts against them): int64, of the broadcast shape.  numpy only.  The
    definition is include/splendor_ppo.h's: eight rounds of an alternating Feistel network over the bits that
    hold n - 1, Philox4x32-10 keyed by the seed and counted by (half, round, draw) as the round function,
    repeated while the value is not below n."""
    n = int(n)
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError("n must be in 1 .. 2^31 - 1")
    pos, drw = np.broadcast_arrays(np.asarray(positions), np.asarray(draw, dtype=np.uint64))
    if pos.size and (pos.min() < 0 or pos.max() >= n):
        raise ValueError("positions must be in [0, n)")
    x = pos.astype(np.uint64).ravel()
    if n == 1:
        return x.astype(np.int64).reshape(pos.shape)
    U, M32 = np.uint64, np.uint64(0xFFFFFFFF)
    d_lo, d_hi = drw.ravel() & M32, drw.ravel() >> U(32)
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = U(seed & 0xFFFFFFFF), U(seed >> 32)
    bits = max(2, (n - 1).bit_length())
    a = bits // 2
    b = bits - a
    todo = np.arange(x.size)  # the elements still walking
    while todo.size:
        y, lo, hi = x[todo], d_lo[todo], d_hi[todo]
        for r in range(8):
            wl, wr = (b, a) if r % 2 == 0 else (a, b)
            L, R = y >> U(wr), y & U((1 << wr) - 1)
            f = _philox4x32_x(R, np.full_like(R, r), lo, hi, np.full_like(R, k0), np.full_like(R, k1))
            y = (R << U(wl)) | ((L ^ f) & U((1 << wl) - 1))
        x[todo] = y
        todo = todo[y >= U(n)]
    return x.astype(np.int64).reshape(pos.shape)


def permutation_reference(n, seed, draw):
    """The permutation of 0 .. n-1 that spl_ppo_permute (DevicePermutation.draw) writes for (seed, draw), bit
    for bit, as int64 [n]: element i is the store position that place i of the epoch holds, and minibatch m of
    size B is [m * B : (m + 1) * B].  numpy only, no GPU: a run's seed and DevicePermutation.counter() are
    enough to say afterwards what every minibatch held."""
    draw = int(draw)
    if not 0 <= draw < 2 ** 64:
        raise ValueError("draw must be in 0 .. 2^64 - 1")
    return permutation_positions(np.arange(int(n), dtype=np.int64), n, seed, draw)


class _OnDevice:
    """What the store, DeviceAdam and DeviceNets share: `torch`, `device`, and the stream their calls go to."""

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)


class PPOLossOut:
    """Device views of one spl_ppo_loss_out_t: loss, policy_loss, value_loss, entropy, approx_kl, clipfrac
    (0-dim float64), loss32 (float32) and bad (the bad rows of the call, int32).  `buf` is the struct as
    float64 [7]; the views follow whatever the store's next loss() call with the same B writes there."""
    STATS = ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac")

    def __init__(self, buf, torch):
        self.buf = buf
        for i, name in enumerate(self.STATS):
            setattr(self, name, buf[i])
        self.loss32 = buf.view(torch.float32)[2 * len(self.STATS)]
        self.bad = buf.view(torch.int32)[2 * len(self.STATS) + 1]


_LOSS_FUNCTION = None


def _loss_function(torch):
    """The autograd node of PPORolloutStore.loss (torch is imported when a store is built, not with
    this module)."""
    global _LOSS_FUNCTION
    if _LOSS_FUNCTION is None:
        class PpoLossFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, logits, value, store, idx, coef, normalize):
                ctx.bufs = store._launch_loss(idx, logits, value, coef, normalize)
                ctx.serial, ctx.value_shape = ctx.bufs["serial"], value.shape
                return ctx.bufs["out"].loss32.clone()

            @staticmethod
            def backward(ctx, grad):
                if ctx.bufs["serial"] != ctx.serial:
                    raise RuntimeError("PPORolloutStore.loss: a later loss() call with the same B has overwritten "
                                       "the gradients of this one")
                return grad * ctx.bufs["dlogits"], (grad * ctx.bufs["dvalue"]).view(ctx.value_shape), None, None, None, None

        _LOSS_FUNCTION = PpoLossFunction
    return _LOSS_FUNCTION


class PPORolloutStore(_OnDevice):
    """Step-major planes of one rollout (num_steps x num_envs), as torch tensors on `device`:
    obs_u8 uint8 [K, T, 300], mask_bits int64 [K, T] (the uint64 words of the ABI), action int32,
    logprob / value / reward / adv / ret float32, done uint8 [K, T]; last_value float32 [T] (the
    bootstrap value collect() leaves); errors int64 [1] (bad positions seen by gather)."""

    def __init__(self, num_steps, num_envs, device):
        torch = _native.require_gpu()
        self.torch = torch
        self.lib = _native.load_library()
        K, T = int(num_steps), int(num_envs)
        if K < 1 or T < 1:
            raise ValueError("num_steps and num_envs must be positive")
        self.num_steps, self.num_envs = K, T
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PPORolloutStore lives on a GPU (no CPU fallback)")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.obs_u8 = z((K, T, OBS_U8), torch.uint8)
        self.mask_bits = z((K, T), torch.int64)
        self.action = z((K, T), torch.int32)
        self.logprob, self.value, self.reward = (z((K, T), torch.float32) for _ in range(3))
        self.done = z((K, T), torch.uint8)
        self.adv, self.ret = z((K, T), torch.float32), z((K, T), torch.float32)
        self.last_value = z((T,), torch.float32)
        self.errors = z((1,), torch.int64)
        self._entropy = z((T,), torch.float32)  # act() writes it; the update recomputes the entropy
        self._stats = z((6,), torch.float64)    # spl_ppo_stats_t: count, sum, sumsq, mean, std, {mean32, std32}
        self.mean32 = self._stats.view(torch.float32)[10:11]  # device views for tests and sharded all-reduces
        self.std32 = self._stats.view(torch.float32)[11:12]
        self._scratch = z((int(check(self.lib, self.lib.spl_ppo_gae_scratch_bytes(T))) // 8,), torch.float64)
        self._loss_bufs = {}  # B -> the buffers of loss(): scratch, dlogits, dvalue, out, the call serial
        self._loss_coef = z((4,), torch.float32)  # clip_coef, vclip, vf_coef, ent_coef where spl_ppo_loss_dev reads them
        self.loss_coef = (0.0, 0.0, 0.0, 0.0)     # what the host last wrote there

    def _record(self, **kw):
        with self.torch.cuda.device(self.device):
            check(self.lib, self.lib.spl_ppo_record(self.num_envs, ctypes.byref(PpoRecord(**kw)), self._stream()))

    def record_pre(self, k, obs_u8, mask):
        """Row k's observation (the compact uint8 [T, 300] rows) and legal mask (int8 [T, 45], nonzero =
        legal): call before the dual step that consumes them."""
        t, T = self.torch, self.num_envs
        _tensor(obs_u8, "obs_u8", (t.uint8,), (T, OBS_U8), self.device)
        _tensor(mask, "mask", (t.int8, t.uint8, t.bool), (T, NUM_ACTIONS), self.device)
        self._record(obs_u8=obs_u8.data_ptr(), dst_obs_u8=self.obs_u8[k].data_ptr(), mask=mask.data_ptr(),
                     dst_mask_bits=self.mask_bits[k].data_ptr())

    def record_post(self, k, reward, done):
        """Row k's reward (float32 [T]) and done (one byte per table) as the dual step returned them."""
        t, T = self.torch, self.num_envs
        _tensor(reward, "reward", (t.float32,), (T,), self.device)
        _tensor(done, "done", (t.uint8, t.bool, t.int8), (T,), self.device)
        self._record(reward=reward.data_ptr(), dst_reward=self.reward[k].data_ptr(), done=done.data_ptr(),
                     dst_done=self.done[k].data_ptr())

    def row(self, k):
        """The out= dict that points FusedActorCritic.act at row k (value as the [T, 1] view)."""
        return {"action": self.action[k], "logprob": self.logprob[k], "value": self.value[k].view(self.num_envs, 1),
                "entropy": self._entropy}

    def compute_gae(self, last_value=None, gamma=0.999, gae_lambda=0.95):
        """adv, ret and the advantage statistics (asynchronous).  last_value: float32 [T] or [T, 1], the
        critic's value after the last step (default: self.last_value, which collect() fills)."""
        t, T = self.torch, self.num_envs
        lv = self.last_value if last_value is None else last_value
        if lv.dim() == 2 and lv.shape[1] == 1:
            lv = lv.view(-1)
        _tensor(lv, "last_value", (t.float32,), (T,), self.device)
        a = PpoGae(reward=self.reward.data_ptr(), value=self.value.data_ptr(), done=self.done.data_ptr(),
                   last_value=lv.data_ptr(), adv=self.adv.data_ptr(), ret=self.ret.data_ptr(), gamma=float(gamma),
                   lam=float(gae_lambda), stats=self._stats.data_ptr(), scratch=self._scratch.data_ptr())
        with t.cuda.device(self.device):
            check(self.lib, self.lib.spl_ppo_gae(self.num_steps, T, ctypes.byref(a), self._stream()))
        self._keep = lv
        return self.adv, self.ret

    def stats(self):
        """The statistics of the last compute_gae as Python numbers (synchronises): count, sum, sumsq,
        mean, std (float64; n-1 denominator) and mean32, std32 (their float32 roundings)."""
        s = self._stats.cpu()
        f = s.view(self.torch.float32)
        return {"count": int(s.view(self.torch.int64)[0]), "sum": float(s[1]), "sumsq": float(s[2]), "mean": float(s[3]),
                "std": float(s[4]), "mean32": float(f[10]), "std32": float(f[11])}

    def gather(self, idx, normalize=True, out=None):
        """The minibatch of flat positions idx (int64 [B], k * T + t): obs float32 [B, 297], mask float32
        [B, 45], action int64 [B], logprob / value / adv / ret float32 [B].  adv is normalised with the
        store's mean32 / std32 on the device when `normalize`.  A position outside the store leaves its
        rows as they were and counts in self.errors."""
        t = self.torch
        B = _positions(idx, self.device)
        if out is None:
            e = lambda shape, dt: t.empty(shape, dtype=dt, device=self.device)
            out = {"obs": e((B, OBS_DIM), t.float32), "mask": e((B, NUM_ACTIONS), t.float32), "action": e((B,), t.int64),
                   "logprob": e((B,), t.float32), "value": e((B,), t.float32), "adv": e((B,), t.float32),
                   "ret": e((B,), t.float32)}
        else:
            _tensor(out["obs"], "out['obs']", (t.float32,), (B, OBS_DIM), self.device)
            _tensor(out["mask"], "out['mask']", (t.float32,), (B, NUM_ACTIONS), self.device)
            _tensor(out["action"], "out['action']", (t.int64,), (B,), self.device)
            for name in ("logprob", "value", "adv", "ret"):
                _tensor(out[name], f"out['{name}']", (t.float32,), (B,), self.device)
        a = PpoGather(K=self.num_steps, T=self.num_envs, normalize=1 if normalize else 0, reserved=0,
                      idx=idx.data_ptr(), obs_u8=self.obs_u8.data_ptr(), mask_bits=self.mask_bits.data_ptr(),
                      action=self.action.data_ptr(), logprob=self.logprob.data_ptr(), value=self.value.data_ptr(),
                      adv=self.adv.data_ptr(), ret=self.ret.data_ptr(), stats=self._stats.data_ptr(),
                      out_obs=out["obs"].data_ptr(), out_mask=out["mask"].data_ptr(),
                      out_action=out["action"].data_ptr(), out_logprob=out["logprob"].data_ptr(),
                      out_value=out["value"].data_ptr(), out_adv=out["adv"].data_ptr(), out_ret=out["ret"].data_ptr(),
                      errors=self.errors.data_ptr())
        with t.cuda.device(self.device):
            check(self.lib, self.lib.spl_ppo_gather(B, ctypes.byref(a), self._stream()))
        return out

    def _loss_buffers(self, B):
        bufs = self._loss_bufs.get(B)
        if bufs is None:
            t = self.torch
            e = lambda shape, dt: t.empty(shape, dtype=dt, device=self.device)
            scratch = e((int(check(self.lib, self.lib.spl_ppo_loss_scratch_bytes(B))) // 8,), t.float64)
            bufs = {"scratch": scratch, "dlogits": e((B, NUM_ACTIONS), t.float32), "dvalue": e((B,), t.float32),
                    "out": PPOLossOut(t.zeros(ctypes.sizeof(PpoLossOut) // 8, dtype=t.float64, device=self.device), t),
                    "serial": 0}
            self._loss_bufs[B] = bufs
        return bufs

    def set_loss_coef(self, clip_coef, vclip, vf_coef, ent_coef):
        """The four coefficients into the device block that the device-coefficient loss entry (spl_ppo_loss_dev)
        reads: one small asynchronous copy on the current stream.  Nothing of them is a kernel argument there, so
        a captured loss call follows the block.  ent_coef is signed as spl_ppo_loss_t's is.  A negative
        clip_coef, vclip or vf_coef is not refused here: the device then counts every row of a call as bad."""
        t = self.torch
        self.loss_coef = tuple(float(x) for x in (clip_coef, vclip, vf_coef, ent_coef))
        self._loss_coef.copy_(t.tensor(self.loss_coef, dtype=t.float32), non_blocking=True)

    def _launch_loss(self, idx, logits, value, coef, normalize, device_coef=False):
        """device_coef: the coefficients are the device block's (set_loss_coef), `coef` is not read."""
        bufs = self._loss_buffers(idx.numel())
        if device_coef:
            if not _native.has_permute(self.lib):
                raise RuntimeError(f"the device coefficient block needs spl_ppo_loss_dev (SPL_PPO_PERMUTE), which "
                                   f"{_native.lib_path()} does not export; rebuild the library")
            coef = (0.0, 0.0, 0.0, 0.0)
        a = PpoLoss(K=self.num_steps, T=self.num_envs, normalize=1 if normalize else 0, reserved=0,
                    idx=idx.data_ptr(), mask_bits=self.mask_bits.data_ptr(), action=self.action.data_ptr(),
                    logprob=self.logprob.data_ptr(), value=self.value.data_ptr(), adv=self.adv.data_ptr(),
                    ret=self.ret.data_ptr(), stats=self._stats.data_ptr(), logits=logits.data_ptr(),
                    new_value=value.data_ptr(), clip_coef=coef[0], vclip=coef[1], vf_coef=coef[2], ent_coef=coef[3],
                    dlogits=bufs["dlogits"].data_ptr(), dvalue=bufs["dvalue"].data_ptr(),
                    out=bufs["out"].buf.data_ptr(), errors=self.errors.data_ptr(), scratch=bufs["scratch"].data_ptr())
        with self.torch.cuda.device(self.device):
            if device_coef:
                check(self.lib, self.lib.spl_ppo_loss_dev(idx.numel(), ctypes.byref(a), self._loss_coef.data_ptr(), self._stream()))
            else:
                check(self.lib, self.lib.spl_ppo_loss(idx.numel(), ctypes.byref(a), self._stream()))
        bufs["serial"] += 1
        return bufs

    def loss(self, idx, logits, value, clip_coef=0.2, vclip=0.2, vf_coef=0.5, ent_coef=0.03, entropy_bonus=False,
             normalize=True):
        """The loss head of ppo_update as one device call (spl_ppo_loss), forward and backward: idx int64 [B]
        as for gather, logits float32 [B, 45] (the actor's raw output for those positions' observations),
        value float32 [B] or [B, 1] (the critic's).  The recorded mask, action, log-probability, value,
        advantage (normalised when `normalize`) and return are read from the store's planes.

        Returns (loss, out).  loss is a 0-dim float32 tensor whose backward() hands d loss / d logits and
        d loss / d value to `logits` and `value`.  out (PPOLossOut) holds device views of loss,
        policy_loss, value_loss, entropy, approx_kl, clipfrac (float64) and bad; reading them does not
        synchronise until a value is taken to the host.

        The gradients, the statistics and the scratch live in buffers the store owns, one set per B, sized
        on first use: out, and a pending backward(), belong to the latest loss() call with that B (a
        backward() after a later call raises).  A position outside the store, or a recorded action outside
        its mask, is a bad row: zero gradients, left out of the means (which still divide by B), counted
        in self.errors and out.bad."""
        t = self.torch
        B = _positions(idx, self.device)
        _tensor(logits, "logits", (t.float32,), (B, NUM_ACTIONS), self.device)
        _tensor(value, "value", (t.float32,), (B,), self.device, or_shape=(B, 1))
        coef = (float(clip_coef), float(vclip), float(vf_coef), -float(ent_coef) if entropy_bonus else float(ent_coef))
        return _loss_function(t).apply(logits, value, self, idx, coef, bool(normalize)), self._loss_buffers(B)["out"]

    def minibatches(self, batch_size, generator=None):
        """One epoch's index tensors: a device randperm of the K * T positions split into pieces of
        batch_size, the last one shorter (ppo_splendor.py:334-336)."""
        total = self.num_steps * self.num_envs
        bs = min(int(batch_size), total)
        perm = self.torch.randperm(total, device=self.device, generator=generator)
        for start in range(0, total, bs):
            yield perm[start:start + bs]


def _iterations(env, agent_k, store, mask, seed, table0):
    obs = None
    for k in range(store.num_steps):
        store.record_pre(k, env.agent_obs_u8, mask)
        action = agent_k.act(env.agent_obs_u8, mask, seed=seed, table0=table0, ply_base=env._step_counter,
                             out=store.row(k))[0]
        obs, reward, _, _, done, info = env.dual_step(action)
        mask = info["action_mask"]
        store.record_post(k, reward, done)
    agent_k.get_value(obs, out=store.last_value.view(store.num_envs, 1))
    return obs, mask


def collect(env, agent_k, store, obs, mask, seed=0, table0=0, graph=False):
    """store.num_steps iterations of the config-5 loop (tools/bench_selfplay.py): FusedActorCritic.act on
    env.agent_obs_u8 with the env's device step counter as ply_base, written straight into row k of the
    store, then env.dual_step; observation, mask, reward and done recorded around it.  Afterwards
    store.last_value holds agent_k.get_value of the final observations (the bootstrap value of
    ppo_splendor.py:302).  Returns the new (obs, mask).

    env: a DualStepVectorEnv built with agent_obs_u8=True and a step_counter; obs / mask: what its
    reset() or the previous collect() returned (the env's own buffers).

    graph=True runs the first call eagerly, captures the K iterations as one linear, single-stream
    hipGraph, and replays it on later calls.  The agent's draws are keyed by the device step counter, so a replay draws
    what the eager loop would.  A device-policy opponent ("random", ...) takes its ply from the host, which
    a replay cannot advance, so graph=True refuses it.  A capture holds the opponent pool's size: it is
    taken again after add_snapshot() changed it."""
    torch = store.torch
    if env.agent_obs_u8 is None or env._step_counter is None:
        raise ValueError("collect needs a DualStepVectorEnv built with agent_obs_u8=True and a step_counter")
    if env.num_envs != store.num_envs:
        raise ValueError("the store and the env must hold the same number of tables")
    if obs.data_ptr() != env.eng.obs.data_ptr() or mask.data_ptr() != env.eng.mask.data_ptr():
        raise ValueError("obs and mask must be the env's own buffers (what reset() or collect() returned)")
    with torch.no_grad():
        if not graph:
            return _iterations(env, agent_k, store, mask, seed, table0)
        if isinstance(env.opponent, str):
            raise ValueError("collect(graph=True) needs a network opponent: a device-policy opponent's draws are keyed "
                             "by a host-side ply that a replayed graph would repeat")
        pool = env.pool
        key = (id(env), id(agent_k), int(seed), int(table0), None if pool is None else (len(pool.pool), pool.n_images))
        cached = getattr(store, "_graph", None)
        if cached is not None and cached[0] == key:
            cached[1].replay()
            store._replays += 1
            return cached[2]
        # the first call runs eagerly (it loads every kernel and sizes every buffer, which a capture must
        # not do) and then captures the same K iterations for the calls after it; capturing runs nothing
        out = _iterations(env, agent_k, store, mask, seed, table0)
        torch.cuda.synchronize(store.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _iterations(env, agent_k, store, mask, seed, table0)
        store._graph, store._replays = (key, g, out), 0
        return out


def adam_state_dict(template, step, exp_avg, exp_avg_sq):
    """torch.optim.Adam's state_dict for moments kept elsewhere: `template` is the state_dict of a fresh
    torch.optim.Adam over the same parameters (it supplies param_groups with the installed torch's keys),
    exp_avg / exp_avg_sq one tensor per parameter, step the number of steps taken.  Like torch, no step
    taken means no per-parameter state."""
    import torch
    state = {}
    if step > 0:
        for i, (m, v) in enumerate(zip(exp_avg, exp_avg_sq)):
            state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    return {"state": state, "param_groups": template["param_groups"]}


def adam_state_of(state_dict, shapes):
    """The reverse of adam_state_dict for parameters of `shapes`: (step, exp_avg list, exp_avg_sq list,
    param group).  ValueError for anything DeviceAdam does not do (several groups, weight decay, amsgrad,
    maximize), for moments of another shape and for parameters that disagree about the step; a parameter
    without state has taken no step."""
    groups = state_dict["param_groups"]
    if len(groups) != 1:
        raise ValueError("DeviceAdam holds one parameter group")
    g = groups[0]
    if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
        raise ValueError("DeviceAdam has no weight decay, no amsgrad and does not maximise")
    if list(g["params"]) != list(range(len(shapes))):
        raise ValueError(f"the state_dict is for {len(g['params'])} parameters, not {len(shapes)}")
    state = state_dict["state"]
    steps = {int(float(state[i]["step"])) if i in state else 0 for i in range(len(shapes))}
    if len(steps) != 1:
        raise ValueError(f"the parameters disagree about the step: {sorted(steps)}")
    ms, vs = [], []
    for i, shape in enumerate(shapes):
        m, v = (state[i]["exp_avg"], state[i]["exp_avg_sq"]) if i in state else (None, None)
        for x in (m, v):
            if x is not None and tuple(x.shape) != tuple(shape):
                raise ValueError(f"parameter {i}: moments of shape {tuple(x.shape)} for a parameter of shape {tuple(shape)}")
        ms.append(m)
        vs.append(v)
    return steps.pop(), ms, vs, g


class DeviceAdam(_OnDevice):
    """clip_grad_norm_, torch.optim.Adam.step and the target-KL early stop as one device call per minibatch
    (spl_ppo_adam, include/splendor_ppo.h).  The parameters and their gradients stay where torch put them;
    the two moments live in arenas this object owns, and the hyper-parameters, the step count, the gate's
    latch and the counters in a small state block on the device, so nothing here waits for the device
    except read_state(), state_dict() and load_state_dict().

    params: at most 16 contiguous float32 tensors on one GPU (ValueError otherwise).  max_grad_norm None
    or negative: no clipping.  target_kl <= 0: no gate.  With a gate, a step whose KL exceeds target_kl is
    applied and the steps after it are skipped (and counted in `gated`) until begin_epoch() or
    begin_update(), which is the reference's `break` without the host reading the KL."""

    def __init__(self, params, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, target_kl=0.0):
        torch = _native.require_gpu()
        self.torch, self.lib = torch, _native.load_library()
        self.params = list(params)
        if not 1 <= len(self.params) <= _native.PPO_ADAM_MAX_TENSORS:
            raise ValueError(f"DeviceAdam takes 1 to {_native.PPO_ADAM_MAX_TENSORS} parameter tensors, not {len(self.params)}")
        self.device = self.params[0].device if isinstance(self.params[0], torch.Tensor) else None
        for i, p in enumerate(self.params):
            _tensor(p, f"parameter {i}", (torch.float32,), None, self.device)
            if p.numel() < 1 or p.device.type != "cuda":
                raise ValueError(f"parameter {i} must be a non-empty tensor on a GPU (no CPU fallback)")
        self._at, total = [], 0
        for p in self.params:
            self._at.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.numel = sum(p.numel() for p in self.params)
        self.arena_floats = total
        scratch = int(check(self.lib, self.lib.spl_ppo_adam_scratch_bytes(self.numel)))
        self._scratch = torch.empty(scratch // 8, dtype=torch.float64, device=self.device)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = -1.0 if max_grad_norm is None else float(max_grad_norm)
        self.target_kl = float(target_kl)
        host = _native.PpoAdamState(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                    max_norm=self.max_grad_norm, target_kl=self.target_kl)
        self._state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.float64).to(self.device)
        self._state_i64 = self._state.view(torch.int64)
        a = _native.PpoAdam(n=len(self.params), reserved=0, state=self._state.data_ptr(), scratch=self._scratch.data_ptr())
        for i, p in enumerate(self.params):
            a.numel[i] = p.numel()
        self._args = a
        self._place_arenas(torch.zeros(total, dtype=torch.float32, device=self.device),
                           torch.zeros(total, dtype=torch.float32, device=self.device))

    def _place_arenas(self, exp_avg, exp_avg_sq):
        """The two moment arenas: contiguous float32 [arena_floats] on the device, segment i at the sum of the
        earlier segments' sizes, each rounded up to a multiple of 4."""
        for x in (exp_avg, exp_avg_sq):
            _tensor(x, "an arena", (self.torch.float32,), (self.arena_floats,), self.device)
        self._exp_avg, self._exp_avg_sq = exp_avg, exp_avg_sq
        self._args.exp_avg, self._args.exp_avg_sq = exp_avg.data_ptr(), exp_avg_sq.data_ptr()

    def _set(self, field, value, integer=False):
        """One asynchronous small write into the state block (a captured step() reads the block, so it
        follows the write)."""
        word = getattr(_native.PpoAdamState, field).offset // 8
        (self._state_i64 if integer else self._state)[word:word + 1].fill_(value)

    def set_lr(self, lr):
        self.lr = float(lr)
        self._set("lr", self.lr)

    def set_betas(self, betas):
        self.betas = (float(betas[0]), float(betas[1]))
        self._set("beta1", self.betas[0])
        self._set("beta2", self.betas[1])

    def set_eps(self, eps):
        self.eps = float(eps)
        self._set("eps", self.eps)

    def set_max_grad_norm(self, max_grad_norm):
        self.max_grad_norm = -1.0 if max_grad_norm is None else float(max_grad_norm)
        self._set("max_norm", self.max_grad_norm)

    def set_target_kl(self, target_kl):
        self.target_kl = float(target_kl)
        self._set("target_kl", self.target_kl)

    def _begin(self, what):
        with self.torch.cuda.device(self.device):
            check(self.lib, self.lib.spl_ppo_adam_begin(self._state.data_ptr(), what, self._stream()))

    def begin_update(self):
        """A new update: re-arms the gate and clears applied, gated, nonfinite and `first` (asynchronous)."""
        self._begin(_native.PPO_ADAM_UPDATE)

    def begin_epoch(self):
        """A new epoch: re-arms the gate (asynchronous)."""
        self._begin(_native.PPO_ADAM_EPOCH)

    def step(self, loss_out=None, approx_kl=None):
        """One call on the current stream with every p.grad as it stands, then p.grad = None: gradients are
        taken, never accumulated into, so there is no zero_grad launch.  approx_kl: this minibatch's KL for
        the gate, a one-element float64 (or float32, converted) tensor on the device; default:
        loss_out.approx_kl.  loss_out: a PPOLossOut to latch into `first` / `last` when the step is applied.
        A missing, non-contiguous or non-float32 gradient raises before anything is launched."""
        t, a = self.torch, self._args
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise ValueError(f"parameter {i} has no gradient")
            _tensor(g, f"the gradient of parameter {i}", (t.float32,), p.shape, self.device)
            a.param[i], a.grad[i] = p.data_ptr(), g.data_ptr()
        if approx_kl is not None:
            if not isinstance(approx_kl, t.Tensor) or approx_kl.numel() != 1 or approx_kl.device != self.device or \
                    approx_kl.dtype not in (t.float32, t.float64):
                raise ValueError(f"approx_kl must be a one-element float64 or float32 tensor on {self.device}")
            approx_kl = approx_kl.detach().to(t.float64).contiguous()
        if loss_out is not None and (not isinstance(loss_out, PPOLossOut) or loss_out.buf.device != self.device):
            raise ValueError(f"loss_out must be a PPOLossOut on {self.device}")
        a.approx_kl = None if approx_kl is None else approx_kl.data_ptr()
        a.loss_out = None if loss_out is None else loss_out.buf.data_ptr()
        with t.cuda.device(self.device):
            check(self.lib, self.lib.spl_ppo_adam(ctypes.byref(a), self._stream()))
        for p in self.params:
            p.grad = None

    def read_state(self):
        """The state block as Python numbers (one synchronising read): step, applied, gated, nonfinite,
        stopped, active, grad_norm, clip_coef, the hyper-parameters as the device holds them, and first /
        last as dictionaries of loss, policy_loss, value_loss, entropy, approx_kl, clipfrac and bad."""
        s = _native.PpoAdamState.from_buffer_copy(self._state.cpu().numpy().tobytes())
        latch = lambda o: {**{k: float(getattr(o, k)) for k in PPOLossOut.STATS}, "bad": int(o.bad)}
        res = {k: int(getattr(s, k)) for k in ("step", "applied", "gated", "nonfinite", "stopped", "active")}
        res.update({k: float(getattr(s, k)) for k in ("grad_norm", "clip_coef", "lr", "beta1", "beta2", "eps", "max_norm", "target_kl")})
        return {**res, "first": latch(s.first), "last": latch(s.last)}

    def _moments(self, arena):
        return [arena[at:at + p.numel()].view(p.shape) for at, p in zip(self._at, self.params)]

    def _template(self):
        t = self.torch
        shells = [t.nn.Parameter(t.empty(0)) for _ in self.params]
        return t.optim.Adam(shells, lr=self.lr, betas=self.betas, eps=self.eps).state_dict()

    def state_dict(self):
        """torch.optim.Adam's own format (state[i] = {step, exp_avg, exp_avg_sq}, param_groups), so that a
        run can move between the two optimisers.  max_grad_norm and target_kl are not part of it.
        Synchronises."""
        step = int(self._state_i64[_native.PpoAdamState.step.offset // 8].item())
        return adam_state_dict(self._template(), step, self._moments(self._exp_avg), self._moments(self._exp_avg_sq))

    def load_state_dict(self, state_dict):
        """Takes a torch.optim.Adam (or DeviceAdam) state_dict for the same parameters: the moments, the step
        and the group's lr, betas and eps."""
        step, ms, vs, group = adam_state_of(state_dict, [p.shape for p in self.params])
        for arena, src in ((self._exp_avg, ms), (self._exp_avg_sq, vs)):
            for dst, x in zip(self._moments(arena), src):
                if x is None:
                    dst.zero_()
                else:
                    dst.copy_(x.to(device=self.device, dtype=self.torch.float32))
        self._set("step", step, integer=True)
        self.set_lr(group["lr"])
        self.set_betas(group["betas"])
        self.set_eps(group["eps"])


class DeviceNets(_OnDevice):
    """The actor's and the critic's forward and backward passes of the update as device calls
    (spl_ppo_net_forward / spl_ppo_net_backward, include/splendor_ppo.h): no autograd graph, no gathered
    float observations, no zero_grad.  `agent` is an ActorCritic whose twelve parameters are float32,
    contiguous, of the reference's shapes (297 -> 256 -> 256 -> 45 | 1) and on one GPU; anything else is a
    ValueError (there is no CPU fallback).  The parameters stay where torch put them and are read in place, so
    optimiser steps and load_state_dict are seen by the next call.

    A parameter without a .grad gets one here, once; backward() OVERWRITES every p.grad (and puts its own
    tensor back where an optimiser has set p.grad to None), so a DeviceAdam or a torch.optim optimiser over
    the same parameters reads the gradients in place.  The outputs, the saved activations and the scratch
    are kept per B, sized on first use: what forward() returned belongs to the latest call with that B.

    `tiled` chooses between the two pairs of calls, which give the same bytes in the same buffers: False
    (the default) the 8-rows-a-workgroup passes built for minibatches of a few hundred rows, True the
    LDS-tiled matrix-core passes (spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled) built for tens of
    thousands, "auto" the tiled ones from TILED_MIN_ROWS rows upward.  A library without the tiled calls is
    a RuntimeError for anything but False.

    `operands` chooses the number format of the matrix products: "f32" (the default) the two pairs above,
    "bf16" the opt-in mixed-precision pair (spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16): both
    operands of every matrix-core product rounded to bf16, float32 accumulation, float32 master weights and
    everything elementwise in float32, the inputs exact.  It is used at every B and `tiled` is then not
    consulted, so a run's numbers do not depend on the minibatch size; they do differ from an "f32" run's.
    A library without SPL_PPO_NET_BF16 is a RuntimeError."""
    MAX_ROWS = _native.PPO_NET_MAX_ROWS
    TILE_ROWS = _native.PPO_NET_TILE_ROWS
    TILED_MIN_ROWS = 4096  # the smallest benchmarked B at which the tiled passes beat the others (profiles/ppo/bench_ppo_nets_tiled.json)

    def __init__(self, agent, tiled=False, operands="f32"):
        import torch
        if not any(tiled is v for v in (False, True)) and tiled != "auto":
            raise ValueError(f"tiled must be False, True or 'auto', not {tiled!r}")
        if not isinstance(operands, str) or operands not in ("f32", "bf16"):
            raise ValueError(f"operands must be 'f32' or 'bf16', not {operands!r}")
        nets = []
        for name, n3 in (("actor", NUM_ACTIONS), ("critic", 1)):
            net = getattr(agent, name, None)
            if not isinstance(net, torch.nn.Sequential) or len(net) != 5 or \
                    not all(isinstance(net[i], torch.nn.Linear) and net[i].bias is not None for i in (0, 2, 4)):
                raise ValueError(f"agent.{name} must be Sequential(Linear, Tanh, Linear, Tanh, Linear) with biases")
            ps = [net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias]
            H = _native.PPO_NET_HIDDEN
            shapes = ((H, OBS_DIM), (H,), (H, H), (H,), (n3, H), (n3,))
            for p, shape, field in zip(ps, shapes, ("w1", "b1", "w2", "b2", "w3", "b3")):
                _tensor(p, f"{name}.{field}", (torch.float32,), shape)  # wherever it lies: the device is checked below
            nets.append(ps)
        self.torch, self.lib = _native.require_gpu(), _native.load_library()
        self.params = nets[0] + nets[1]  # the actor's six, then the critic's
        self.device = self.params[0].device
        if self.device.type != "cuda" or any(p.device != self.device for p in self.params):
            raise ValueError("DeviceNets needs every parameter on one GPU (no CPU fallback)")
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        self._grads = [p.grad for p in self.params]
        self._bufs = {}
        self.tiled = tiled
        if tiled is not False and not _native.has_net_tiled(self.lib):
            raise RuntimeError(f"DeviceNets(tiled={tiled!r}) needs spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled "
                               f"(SPL_PPO_NET_TILED), which {_native.lib_path()} does not export; rebuild the library")
        self.operands = operands
        if operands == "bf16" and not _native.has_net_bf16(self.lib):
            raise RuntimeError("DeviceNets(operands='bf16') needs spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16 "
                               f"(SPL_PPO_NET_BF16), which {_native.lib_path()} does not export; rebuild the library")

    def _use_tiled(self, B):
        return self.tiled is True or (self.tiled == "auto" and B >= self.TILED_MIN_ROWS)

    def _call(self, which, B):
        """spl_ppo_net_<which> of the pair that takes B rows"""
        suffix = "_bf16" if self.operands == "bf16" else "_tiled" if self._use_tiled(B) else ""
        return getattr(self.lib, f"spl_ppo_net_{which}{suffix}")

    def _mlp(self, tensors):
        return _native.PpoMlp(*(x.data_ptr() for x in tensors))

    def _buffers(self, B):
        bufs = self._bufs.get(B)
        if bufs is None:
            t = self.torch
            e = lambda n: t.empty(n, dtype=t.float32, device=self.device)
            bufs = {"logits": e((B, NUM_ACTIONS)), "value": e((B,)),
                    "act": e(int(check(self.lib, self.lib.spl_ppo_net_act_bytes(B))) // 4),
                    "scratch": e(int(check(self.lib, self.lib.spl_ppo_net_scratch_bytes(B))) // 4)}
            self._bufs[B] = bufs
        return bufs

    def _idx(self, store, idx):
        if store.device != self.device:
            raise ValueError(f"the store must be on {self.device}")
        if _positions(idx, self.device) > self.MAX_ROWS:
            raise ValueError(f"DeviceNets takes at most {self.MAX_ROWS} rows a call (SPL_PPO_NET_MAX_ROWS), not {idx.numel()}")
        return idx if idx.data_ptr() % 16 == 0 else idx.clone()  # a slice of a permutation may start anywhere

    def forward(self, store, idx):
        """(logits float32 [B, 45], value float32 [B]) of the store's flat positions idx (int64 [B], as for
        store.gather), plain tensors this object owns.  A position outside the store gives zeros and
        counts in store.errors.  Asynchronous."""
        idx = self._idx(store, idx)
        B = idx.numel()
        bufs = self._buffers(B)
        a = _native.PpoNetFwd(K=store.num_steps, T=store.num_envs, reserved=0, idx=idx.data_ptr(),
                              obs_u8=store.obs_u8.data_ptr(), actor=self._mlp(self.params[:6]),
                              critic=self._mlp(self.params[6:]), logits=bufs["logits"].data_ptr(),
                              new_value=bufs["value"].data_ptr(), act=bufs["act"].data_ptr(), errors=store.errors.data_ptr())
        with self.torch.cuda.device(self.device):
            check(self.lib, self._call("forward", B)(B, ctypes.byref(a), self._stream()))
        bufs["idx"] = idx
        return bufs["logits"], bufs["value"]

    def backward(self, store, idx, dlogits, dvalue):
        """Every p.grad = the gradient that dlogits (float32 [B, 45]) and dvalue (float32 [B] or [B, 1]) give
        through the two networks, for the latest forward() with this B (same store, same idx, parameters
        untouched since).  Overwrites, never accumulates.  Asynchronous."""
        t = self.torch
        idx = self._idx(store, idx)
        B = idx.numel()
        if B not in self._bufs:
            raise ValueError(f"backward() needs a forward() with the same B = {B} before it")
        bufs = self._bufs[B]
        _tensor(dlogits, "dlogits", (t.float32,), (B, NUM_ACTIONS), self.device)
        _tensor(dvalue, "dvalue", (t.float32,), (B,), self.device, or_shape=(B, 1))
        for p, g in zip(self.params, self._grads):
            if p.grad is None:
                p.grad = g
            else:
                _tensor(p.grad, "every p.grad", (t.float32,), p.shape, self.device)
        grads = [p.grad for p in self.params]
        a = _native.PpoNetBwd(K=store.num_steps, T=store.num_envs, reserved=0, idx=idx.data_ptr(),
                              obs_u8=store.obs_u8.data_ptr(), actor=self._mlp(self.params[:6]),
                              critic=self._mlp(self.params[6:]), dlogits=dlogits.data_ptr(), dvalue=dvalue.data_ptr(),
                              act=bufs["act"].data_ptr(), actor_grad=self._mlp(grads[:6]), critic_grad=self._mlp(grads[6:]),
                              scratch=bufs["scratch"].data_ptr())
        with t.cuda.device(self.device):
            check(self.lib, self._call("backward", B)(B, ctypes.byref(a), self._stream()))
        bufs["idx"] = idx


class DevicePermutation(_OnDevice):
    """An epoch's permutation of `total` store positions drawn on the device (spl_ppo_permute,
    include/splendor_ppo.h) and cut into minibatches of `batch_size` (at most `total`), the last one shorter.
    The state block (seed, draw) lives on the device and draw() advances it there, so a captured draw() gives
    the next permutation on every replay; the permutation for (seed, draw) is permutation_reference's.

    The buffer is [ceil(total / B)][B rounded up to even] int64, the pad word of a row and the last row's tail
    -1, so every view of minibatches() starts 16-byte aligned and DeviceNets never clones it.  A device
    permutation is another permutation than torch.randperm's: a run that switches to it is another run."""

    def __init__(self, total, batch_size, device, seed=0):
        torch = _native.require_gpu()
        self.torch, self.lib = torch, _native.load_library()
        if not _native.has_permute(self.lib):
            raise RuntimeError(f"DevicePermutation needs spl_ppo_permute (SPL_PPO_PERMUTE), which {_native.lib_path()} "
                               "does not export; rebuild the library")
        self.total = int(total)
        if not 1 <= self.total <= 2 ** 31 - 1:
            raise ValueError("total must be in 1 .. 2^31 - 1")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        self.batch_size = B = min(int(batch_size), self.total)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DevicePermutation lives on a GPU (no CPU fallback)")
        self.rows, self.stride = (self.total + B - 1) // B, (B + 1) // 2 * 2
        self._state = torch.zeros(2, dtype=torch.int64, device=self.device)  # spl_ppo_perm_state_t: seed, draw
        self._buf = torch.full((self.rows, self.stride), -1, dtype=torch.int64, device=self.device)
        last = self.total - (self.rows - 1) * B
        self._views = [self._buf[r, :B if r < self.rows - 1 else last] for r in range(self.rows)]
        self._args = _native.PpoPermute(n=self.total, B=B, reserved=0, state=self._state.data_ptr(), out=self._buf.data_ptr())
        self.set_seed(seed)

    @staticmethod
    def _word(x):
        x = int(x) & (2 ** 64 - 1)  # the uint64 word as the int64 torch holds
        return x - 2 ** 64 if x >= 2 ** 63 else x

    def set_seed(self, seed):
        """Asynchronous."""
        self.seed = int(seed) & (2 ** 64 - 1)
        self._state[0:1].fill_(self._word(seed))

    def set_counter(self, draw):
        """The draw counter the next draw() uses, e.g. a resumed run's (asynchronous)."""
        self._state[1:2].fill_(self._word(draw))

    def counter(self):
        """The draw counter: how many draw() calls and replays of one this state has seen since 0
        (synchronises)."""
        return int(self._state[1].item()) & (2 ** 64 - 1)

    def draw(self):
        """The next permutation into the buffer behind minibatches(); the counter advances by one on the device
        (one spl_ppo_permute call, asynchronous)."""
        with self.torch.cuda.device(self.device):
            check(self.lib, self.lib.spl_ppo_permute(ctypes.byref(self._args), self._stream()))

    def minibatches(self):
        """The fixed list of views of the buffer, one per minibatch: contiguous int64, 16-byte aligned, holding
        whatever the latest draw() wrote."""
        return list(self._views)


GRAPH_MAX_MINIBATCHES = 1024  # ppo_update(graph=True): update_epochs x minibatches per epoch at the most


class _Lazy:
    """Attributes given as functions without arguments, each evaluated when it is first read, and kept."""

    def __init__(self, **thunks):
        self._thunks = thunks

    def __getattr__(self, name):
        if name == "_thunks" or name not in self._thunks:
            raise AttributeError(name)
        setattr(self, name, self._thunks.pop(name)())
        return getattr(self, name)


def _result(stat, first_kl, steps, with_clipfrac, **more):
    """ppo_update's dictionary; stat(name): the last applied minibatch's statistic as a Python number."""
    res = {name: stat(name) for name in ("policy_loss", "value_loss", "entropy", "approx_kl")}
    res.update(first_approx_kl=float(first_kl), optimizer_steps=steps)
    if with_clipfrac:
        res["clipfrac"] = stat("clipfrac")
    return {**res, **more}


class _TorchOptimStep:
    """ppo_update's step with a torch.optim optimiser: clip_grad_norm_, step() and, with a target, one read of the
    minibatch's KL.  step(out) says whether the epoch goes on."""
    begin_epoch = staticmethod(lambda: None)

    def __init__(self, torch, agent, optimizer, max_grad_norm, target_kl):
        self.clip = lambda: torch.nn.utils.clip_grad_norm_(agent.parameters(), max_grad_norm)
        self.optimizer, self.zero_grad, self.target_kl = optimizer, optimizer.zero_grad, target_kl
        self.first_kl, self.last, self.steps = None, None, 0

    def step(self, out):
        self.clip()
        self.optimizer.step()
        self.steps += 1
        kl = out.approx_kl  # the torch head's is worked out here, behind the step, whether or not anything reads it
        if self.first_kl is None:  # a PPOLossOut's views follow the next call with the same B
            self.first_kl = kl.clone() if isinstance(out, PPOLossOut) else kl
        self.last = out  # read after the loop, when a PPOLossOut holds the latest call with its B: this one
        return not (self.target_kl > 0 and kl.item() > self.target_kl)

    def result(self):
        return _result(lambda name: float(getattr(self.last, name)), self.first_kl, self.steps,
                       isinstance(self.last, PPOLossOut))


class _DeviceAdamStep:
    """ppo_update's step with a DeviceAdam: the clip, the step and the early stop in DeviceAdam.step, fed the
    minibatch's statistics; nothing is read inside the loop, the optimiser's state once for the result."""
    zero_grad = staticmethod(lambda: None)  # DeviceAdam.step takes the gradients: every p.grad is None by now

    def __init__(self, optimizer, max_grad_norm, target_kl):
        norm = -1.0 if max_grad_norm is None else float(max_grad_norm)
        if optimizer.max_grad_norm != norm:
            optimizer.set_max_grad_norm(norm)
        if optimizer.target_kl != float(target_kl):
            optimizer.set_target_kl(target_kl)
        self.optimizer, self.epochs, self.with_clipfrac = optimizer, 0, False

    def begin_epoch(self):
        (self.optimizer.begin_epoch if self.epochs else self.optimizer.begin_update)()
        self.epochs += 1

    def step(self, out):
        self.with_clipfrac = isinstance(out, PPOLossOut)
        if not self.with_clipfrac:  # the torch head's statistics as one spl_ppo_loss_out_t for the optimiser's latches
            torch = self.optimizer.torch
            stats = [getattr(out, name) for name in PPOLossOut.STATS]
            buf = torch.zeros(ctypes.sizeof(PpoLossOut) // 8, dtype=torch.float64, device=self.optimizer.device)
            buf[:len(stats)] = torch.stack(stats)
            out = PPOLossOut(buf, torch)
        self.optimizer.step(loss_out=out)
        return True  # the device skips the steps behind the crossing; the host runs every minibatch

    def result(self):
        st = self.optimizer.read_state()
        return _result(st["last"].__getitem__, st["first"]["approx_kl"], st["applied"], self.with_clipfrac,
                       gated=st["gated"], grad_norm=st["grad_norm"])


def ppo_update(agent, optimizer, store, clip_coef=0.2, vclip=0.2, ent_coef=0.03, vf_coef=0.5, update_epochs=4,
               minibatch_size=256, target_kl=0.02, max_grad_norm=0.5, generator=None, entropy_bonus=False,
               fused_loss=False, device_nets=False, permutation=None, graph=False):
    """The update of ppo_splendor.py:327-361 over store.minibatches (call store.compute_gae first):
    clipped policy loss, clipped value loss, the entropy term, grad-norm clip at 0.5 and the target-KL
    early stop, which like the reference's `break` ends the current epoch only.

    The reference's loss is policy_loss + vf_coef * value_loss + ent_coef * entropy: its double negation
    (entropy_loss = -entropy; ... + ent_coef * (-entropy_loss)) ADDS the entropy to the minimised loss.
    That is reproduced by default; entropy_bonus=True subtracts it instead (the usual PPO bonus).

    A minibatch is a loss head, which leaves every p.grad and the statistics, then an optimiser step.

    The head.  By default store.gather, agent.get_action_and_value, the loss in torch and backward().
    fused_loss=True replaces everything between the two networks and loss.backward() by store.loss (one
    device call for the loss, its statistics and its gradients); the gather then only supplies the
    observations.  The arithmetic is the same, in another summation order.  device_nets=True (or a DeviceNets
    over this agent, which keeps its buffers from update to update) also moves the two networks' passes to
    the device and implies the fused loss: DeviceNets.forward -> the loss launch -> DeviceNets.backward, with
    no autograd, no gather and no zero_grad.

    The step.  A torch.optim optimiser: zero_grad, clip_grad_norm_, step() and the per-minibatch KL
    read-back.  A DeviceAdam: the norm clip, the Adam step and the early stop are one device call per
    minibatch (DeviceAdam.step, fed the minibatch's KL), with any head: no clip_grad_norm_, no zero_grad and
    no read-back inside the loop, and one synchronising read of the optimiser's state at the end (with the
    nets head: four device calls a minibatch and one read-back per update).  max_grad_norm and target_kl are
    this call's arguments: the optimiser's own are set to them when they differ.  Since the host no longer
    learns that the KL crossed the line, it runs every minibatch of every epoch, and a minibatch behind the
    crossing still pays for its head before its step is skipped on the device: the price of not synchronising.

    Returns the last minibatch's policy_loss, value_loss, entropy and approx_kl, first_approx_kl (the
    first minibatch's, evaluated before any optimiser step) and optimizer_steps; with the fused or the nets
    head also the last minibatch's clipfrac.  With a DeviceAdam the dictionary is filled from the device
    (optimizer_steps = the applied steps, the statistics those of the last applied step, first_approx_kl
    that of the first), plus gated (skipped minibatches) and grad_norm (the last call's).

    The permutation.  By default store.minibatches: torch.randperm from `generator`, once per epoch.
    permutation=DevicePermutation(K * T, minibatch_size, device, seed): every epoch calls permutation.draw()
    and walks its views instead, with any head and either optimiser; `generator` is then not used, and the
    minibatches are permutation_reference's for the counters the update passed through.  Another permutation
    than torch.randperm's, so another run.

    graph=True (needs a DeviceAdam, device_nets=a DeviceNets object and a DevicePermutation; ValueError
    otherwise) runs the first call eagerly, then captures one whole update on one stream (begin_update; per
    epoch begin_epoch, draw and every minibatch's forward, loss, backward and step) as one linear hipGraph,
    and later calls replay it.  Everything that changes between updates is read from device memory: the draw
    counter, the optimiser's state block (set_lr, max_grad_norm and target_kl are followed) and the four loss
    coefficients, which go through store.set_loss_coef and the device-coefficient loss entry, in the eager
    first call too.  The numbers are those of graph=False with the same permutation, bit for bit.  The
    capture is kept on the store, keyed by what is baked into it (the objects, K, T, minibatch_size,
    update_epochs, the nets' tiled and operands); a changed key captures again.  store._update_replays counts
    the replays since the capture.  More than GRAPH_MAX_MINIBATCHES minibatches an update is refused."""
    torch = store.torch
    epochs = int(update_epochs)
    if epochs < 1:
        raise ValueError("update_epochs must be at least 1")
    if graph:  # refused before anything is built or launched
        if not isinstance(optimizer, DeviceAdam):
            raise ValueError("ppo_update(graph=True) needs a DeviceAdam as the optimizer: a torch.optim step reads the "
                             "minibatch's KL on the host, which a replayed graph cannot do")
        if not isinstance(device_nets, DeviceNets):
            raise ValueError("ppo_update(graph=True) needs device_nets=a DeviceNets object (the nets head, with buffers that "
                             "live from update to update): autograd builds its own graph on every call")
        if not isinstance(permutation, DevicePermutation):
            raise ValueError("ppo_update(graph=True) needs permutation=a DevicePermutation: torch.randperm's generator "
                             "does not advance inside a replayed graph")
    if permutation is not None:
        total = store.num_steps * store.num_envs
        if not isinstance(permutation, DevicePermutation):
            raise ValueError("permutation must be a DevicePermutation or None")
        if permutation.total != total or permutation.batch_size != min(int(minibatch_size), total) or \
                permutation.device != store.device:
            raise ValueError(f"the DevicePermutation is for {permutation.total} positions in minibatches of "
                             f"{permutation.batch_size} on {permutation.device}, the update for {total} in minibatches of "
                             f"{min(int(minibatch_size), total)} on {store.device}")
        if graph and epochs * permutation.rows > GRAPH_MAX_MINIBATCHES:
            raise ValueError(f"ppo_update(graph=True) captures at most GRAPH_MAX_MINIBATCHES = {GRAPH_MAX_MINIBATCHES} "
                             f"minibatches an update, not {epochs} epochs x {permutation.rows}")
    nets = None
    if device_nets is not False and device_nets is not None:
        nets = device_nets if isinstance(device_nets, DeviceNets) else DeviceNets(agent)
        if nets.params[0] is not agent.actor[0].weight or nets.params[6] is not agent.critic[0].weight:
            raise ValueError("device_nets was built over another agent's parameters")
    if isinstance(optimizer, DeviceAdam):
        stepper = _DeviceAdamStep(optimizer, max_grad_norm, target_kl)
    else:
        stepper = _TorchOptimStep(torch, agent, optimizer, max_grad_norm, target_kl)
    coef = (float(clip_coef), float(vclip), float(vf_coef), -float(ent_coef) if entropy_bonus else float(ent_coef))

    def torch_head(idx):
        mb = store.gather(idx, normalize=True)
        _, new_logprob, entropy, new_value = agent.get_action_and_value(mb["obs"], mb["mask"], mb["action"])
        ratio = (new_logprob - mb["logprob"]).exp()
        clip_adv = torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef) * mb["adv"]
        policy_loss = -torch.min(ratio * mb["adv"], clip_adv).mean()
        v_pred = new_value.squeeze(-1)
        v_clipped = mb["value"] + torch.clamp(v_pred - mb["value"], -vclip, vclip)
        value_loss = 0.5 * torch.max((v_pred - mb["ret"]).pow(2), (v_clipped - mb["ret"]).pow(2)).mean()
        entropy = entropy.mean()
        loss = policy_loss + vf_coef * value_loss + coef[3] * entropy
        stepper.zero_grad()
        loss.backward()
        # PPOLossOut's names.  The KL and the clipfrac are launched when read: a torch.optim step reads the KL behind
        # its step() and never the clipfrac, a DeviceAdam reads both before its own
        return _Lazy(loss=loss.detach, policy_loss=policy_loss.detach, value_loss=value_loss.detach, entropy=entropy.detach,
                     approx_kl=lambda: (mb["logprob"] - new_logprob.detach()).mean(),
                     clipfrac=lambda: ((ratio.detach() - 1).abs() > clip_coef).float().mean())

    held = []  # the fused head's observations and loss outlive its call, as they would in a flat loop: with both freed
    # at once an update of 65 536-row minibatches measured 0.2 to 0.5 % slower (the same kernels at other addresses)

    def fused_head(idx):
        obs = store.gather(idx, normalize=True)["obs"]
        loss, out = store.loss(idx, agent.actor(obs), agent.critic(obs), *coef, normalize=True)
        stepper.zero_grad()
        loss.backward()
        held[:] = obs, loss
        return out

    def nets_head(idx):
        logits, value = nets.forward(store, idx)
        bufs = store._launch_loss(idx, logits, value, coef, True, device_coef=bool(graph))
        nets.backward(store, idx, bufs["dlogits"], bufs["dvalue"])  # overwrites every p.grad: no zero_grad
        return bufs["out"]

    head = nets_head if nets is not None else fused_head if fused_loss else torch_head

    def epoch_minibatches():
        if permutation is None:
            return store.minibatches(minibatch_size, generator)
        permutation.draw()
        return permutation.minibatches()

    def update():
        for _ in range(epochs):
            stepper.begin_epoch()
            for idx in epoch_minibatches():
                if not stepper.step(head(idx)):
                    break

    if not graph:
        update()
        return stepper.result()
    # the coefficients, like max_grad_norm and target_kl in the stepper above, are written where they differ from
    # what the device holds, outside the graph
    if store.loss_coef != coef:
        store.set_loss_coef(*coef)
    key = (id(agent), id(optimizer), id(nets), id(permutation), store.num_steps, store.num_envs, permutation.batch_size,
           epochs, True, nets.tiled, nets.operands)
    cached = getattr(store, "_update_graph", None)
    if cached is not None and cached[0] == key:
        stepper.with_clipfrac = True  # the nets head's statistics, as in the eager call
        cached[1].replay()
        store._update_replays += 1
        return stepper.result()
    # as collect(graph=True): the first call runs eagerly (it loads every kernel and sizes every per-B buffer, which
    # a capture must not do) and then captures the same update for the calls after it; capturing runs nothing
    update()
    res = stepper.result()  # synchronises
    torch.cuda.synchronize(store.device)
    stepper.epochs = 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        update()
    store._update_graph, store._update_replays = (key, g, agent, optimizer, nets, permutation), 0
    return res
