"""One PPO update as one replayed graph (splendor_gym.ppo.ppo_update(permutation=, graph=)): the minibatches an
eager update walks are the reference permutation's, and a captured and replayed update is the eager update with
the same device permutation, byte for byte: parameters, moments, the optimiser's state block and the result
dictionary, with ent_coef, the learning rate and the permutation changing from update to update."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_ppo_adam import EPS, LR, bits
from test_gpu_ppo_loss import DEV, trained

pytestmark = pytest.mark.gpu

K, T = 16, 64
P = K * T
SEED = 9


@pytest.fixture(scope="module")
def collected():
    """The committed checkpoint, and a 16 x 64 store it collected against the random opponent, with GAE, filled the
    way test_gpu_ppo_loss.py's fixture fills its own.  The tests only read it."""
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore, collect
    from splendor_gym.selfplay import DualStepVectorEnv
    agent = trained()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    env = DualStepVectorEnv(T, device=DEV, opponent="random", policy_seed=3, opponent_obs=False, step_counter=counter,
                            agent_obs_u8=True)
    obs, info = env.reset(seed=40)
    store = PPORolloutStore(K, T, DEV)
    collect(env, FusedActorCritic(agent), store, obs, info["action_mask"], seed=5)
    store.compute_gae()
    env.close()
    return agent, store


def make(agent, minibatch_size, **nets_kw):
    from splendor_gym.ppo import DeviceAdam, DeviceNets, DevicePermutation
    a = copy.deepcopy(agent)
    return {"agent": a, "nets": DeviceNets(a, **nets_kw), "opt": DeviceAdam(list(a.parameters()), lr=LR, eps=EPS),
            "perm": DevicePermutation(P, minibatch_size, DEV, seed=SEED), "mb": minibatch_size}


def update(run, store, graph, **kw):
    from splendor_gym.ppo import ppo_update
    kw.setdefault("update_epochs", 2)
    return ppo_update(run["agent"], run["opt"], store, minibatch_size=run["mb"], device_nets=run["nets"],
                      permutation=run["perm"], graph=graph, **kw)


def same_bytes(x, y):
    """parameters, both moment arenas, the optimiser's state block, the draw counter"""
    import torch
    got = bits(x["agent"].parameters()) + bits([x["opt"]._exp_avg, x["opt"]._exp_avg_sq])
    want = bits(y["agent"].parameters()) + bits([y["opt"]._exp_avg, y["opt"]._exp_avg_sq])
    return all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == 14 and \
        torch.equal(x["opt"]._state.view(torch.int64), y["opt"]._state.view(torch.int64)) and \
        torch.equal(x["perm"]._state, y["perm"]._state)


def test_eager_update_walks_the_reference_permutation(collected):
    import torch
    from splendor_gym.ppo import permutation_reference
    agent, store = collected
    run = make(agent, 384)
    walked, forward = [], run["nets"].forward

    def recording(s, idx):
        walked.append((idx.data_ptr() % 16, idx.clone()))
        return forward(s, idx)

    run["nets"].forward = recording
    res = update(run, store, False, update_epochs=4, target_kl=0.0)
    assert res["optimizer_steps"] == 12 and len(walked) == 12 and run["perm"].counter() == 4
    assert all(misaligned == 0 for misaligned, _ in walked)  # DeviceNets._idx had nothing to clone
    for epoch in range(4):
        ref = permutation_reference(P, SEED, epoch)
        for m, size in enumerate((384, 384, 256)):
            got = walked[3 * epoch + m][1].cpu().numpy()
            assert np.array_equal(got, ref[384 * m:384 * m + size]), (epoch, m)
    assert int(store.errors.item()) == 0
    # the torch head and torch.optim.Adam walk a device permutation too; another seed is another update
    a = copy.deepcopy(agent)
    from splendor_gym.ppo import ppo_update
    r = ppo_update(a, torch.optim.Adam(a.parameters(), lr=LR, eps=EPS), store, update_epochs=1, minibatch_size=384,
                   target_kl=0.0, permutation=run["perm"])
    assert r["optimizer_steps"] == 3 and run["perm"].counter() == 5


def variants():
    from splendor_gym import _native
    lib = _native.load_library()
    tiled = pytest.mark.skipif(not _native.has_net_tiled(lib), reason="the library has no tiled passes")
    bf16 = pytest.mark.skipif(not _native.has_net_bf16(lib), reason="the library has no bf16 passes")
    return [pytest.param(384, {}, id="384"), pytest.param(341, {}, id="341"),
            pytest.param(384, {"tiled": True}, id="384-tiled", marks=tiled),
            pytest.param(384, {"operands": "bf16"}, id="384-bf16", marks=bf16)]


@pytest.mark.parametrize("minibatch_size,nets_kw", variants())
def test_graph_equals_eager(collected, minibatch_size, nets_kw):
    """Three updates each: one eager call and two replays against three eager calls.  384: minibatches of 384, 384
    and 256; 341: three of 341 and one of a single row (odd stride, B = 1).  ent_coef differs on each update and
    set_lr is called between them, so a frozen coefficient, learning rate or permutation would show."""
    agent, store = collected
    g, e = make(agent, minibatch_size, **nets_kw), make(agent, minibatch_size, **nets_kw)
    start = bits(agent.parameters())
    for k, (ent, lr) in enumerate(((0.03, LR), (0.02, 1e-3), (0.01, 5e-4))):
        for run in (g, e):
            run["opt"].set_lr(lr)
        res_g, res_e = update(g, store, True, ent_coef=ent), update(e, store, False, ent_coef=ent)
        print(f"update {k}: graph {res_g}")
        assert res_g == res_e, (k, res_g, res_e)
        assert same_bytes(g, e), k
        assert store._update_replays == k and g["perm"].counter() == 2 * (k + 1)
        assert store.loss_coef == (0.2, 0.2, 0.5, ent)
    assert store._update_replays == 2
    import torch
    assert not torch.equal(bits(g["agent"].parameters())[0], start[0])  # and steps were taken
    assert res_g["optimizer_steps"] >= 2 and int(store.errors.item()) == 0


def test_the_gate_acts_inside_the_graph(collected):
    """A target_kl below any KL that an applied step leaves behind: the steps behind the crossing are gated on the
    device, epoch by epoch, in the replayed update as in the eager one."""
    agent, store = collected
    g, e = make(agent, 256), make(agent, 256)
    for k in range(2):  # the eager first call, then the replay
        res_g = update(g, store, True, target_kl=1e-9)
        res_e = update(e, store, False, target_kl=1e-9)
        assert res_g == res_e and same_bytes(g, e), k
        assert res_g["gated"] > 0 and 2 <= res_g["optimizer_steps"] < 8 and res_g["gated"] + res_g["optimizer_steps"] == 8
    assert store._update_replays == 1 and g["opt"].target_kl == 1e-9
    # another target is written into the state block outside the graph, which the replay follows
    res_g, res_e = update(g, store, True, target_kl=0.0), update(e, store, False, target_kl=0.0)
    assert res_g == res_e and same_bytes(g, e) and res_g["gated"] == 0 and res_g["optimizer_steps"] == 8
    assert store._update_replays == 2


def test_a_changed_key_captures_again(collected):
    agent, store = collected
    g, e = make(agent, 384), make(agent, 384)
    for epochs, replays in ((2, 0), (2, 1), (3, 0), (3, 1)):
        res_g = update(g, store, True, update_epochs=epochs)
        res_e = update(e, store, False, update_epochs=epochs)
        assert res_g == res_e and same_bytes(g, e), (epochs, replays)
        assert store._update_replays == replays
    assert g["perm"].counter() == 10


def test_too_many_minibatches_are_refused(collected):
    import torch
    from splendor_gym.ppo import GRAPH_MAX_MINIBATCHES
    agent, store = collected
    run = make(agent, 1)
    assert 2 * P > GRAPH_MAX_MINIBATCHES
    state = run["opt"]._state.clone()
    with pytest.raises(ValueError, match="GRAPH_MAX_MINIBATCHES"):
        update(run, store, True)
    assert run["perm"].counter() == 0 and torch.equal(run["opt"]._state, state)  # nothing was launched
    assert all(torch.equal(a, b) for a, b in zip(bits(run["agent"].parameters()), bits(agent.parameters())))
    with pytest.raises(ValueError, match="minibatches of 1"):  # a permutation cut for another minibatch size
        update({**run, "mb": 2}, store, False)


def cli(*flags):
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "splendor-gym_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg] + [x for x in (os.environ.get("PYTHONPATH"),) if x]))
    r = subprocess.run([sys.executable, "-m", "splendor_gym.scripts.ppo_device", *flags, "--num-envs", "64", "--num-steps", "16",
                        "--total-timesteps", "4096", "--minibatch-size", "384"], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("update ")]
    assert len(lines) == 4 and lines[-1].startswith("update 4/4 steps 4096 "), r.stdout[-2000:]
    columns = [re.findall(r"(?:pl|vl|ent|kl) ([-+0-9.einfa]+)", ln) for ln in lines]
    assert all(len(c) == 4 and all(np.isfinite(float(x)) for x in c) for c in columns), lines
    return columns


def test_cli_graph_update():
    """ppo_device --graph-update: four updates (one eager, three replays), every printed loss finite, and the columns
    of the same run without the graph."""
    assert cli("--graph-update") == cli("--device-permutation", "--device-adam", "--device-nets")
