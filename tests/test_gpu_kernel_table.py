"""spl_rollout's kernel table: every forced shape, output mode and player count resolves to its own kernel.

The library builds its launches, its occupancy queries and spl_rollout_kernel_name from one table of kernels
(SPL_ROLLOUT_KERNELS in spl_engine.hip), indexed by [shape][per_step][players - 2].  rocprof rows, bench.py
and other tests key on the names, so the table's order is checked here against the names written out.  Only
the name lookup runs: no kernel is launched beyond engine creation.
"""
import pytest

pytestmark = pytest.mark.gpu

# NAMES[spl_ctx_set_rollout_pipeline mode][per_step][players - 2]
NAMES = {
    0: (("k_rollout<2>", "k_rollout<3>", "k_rollout<4>"),  # one wave per 64 tables: one kernel for both output modes
        ("k_rollout<2>", "k_rollout<3>", "k_rollout<4>")),
    2: (("k_rollout_inplace_2p", "k_rollout_inplace_3p", "k_rollout_inplace_4p"),
        ("k_rollout_store_2p", "k_rollout_store_3p", "k_rollout_store_4p")),
    3: (("k_rollout_inplace_half_2p", "k_rollout_inplace_half_3p", "k_rollout_inplace_half_4p"),
        ("k_rollout_store_half_2p", "k_rollout_store_half_3p", "k_rollout_store_half_4p")),
    4: (("k_rollout_inplace_dealer_2p", "k_rollout_inplace_dealer_3p", "k_rollout_inplace_dealer_4p"),
        ("k_rollout_store_dealer_2p", "k_rollout_store_dealer_3p", "k_rollout_store_dealer_4p")),
    5: (("k_rollout_inplace_dealer2_2p", "k_rollout_inplace_dealer2_3p", "k_rollout_inplace_dealer2_4p"),
        ("k_rollout_store_dealer2_2p", "k_rollout_store_dealer2_3p", "k_rollout_store_dealer2_4p")),
    6: (("k_rollout_inplace_quad_2p", "k_rollout_inplace_quad_3p", "k_rollout_inplace_quad_4p"),
        ("k_rollout_store_quad_2p", "k_rollout_store_quad_3p", "k_rollout_store_quad_4p")),
}


@pytest.mark.parametrize("P", [2, 3, 4])
def test_rollout_kernel_names_by_shape(P):
    from splendor_gym import _native
    from splendor_gym.device import Engine
    eng = Engine(256, P)
    forced = set()
    for mode, names in NAMES.items():
        _native.check(eng.lib, eng.lib.spl_ctx_set_rollout_pipeline(eng.ctx, mode))
        for per_step in (0, 1):
            want = names[per_step][P - 2]
            assert eng.rollout_kernel_name(per_step=bool(per_step)) == want, (mode, per_step)
            forced.add(want)
    _native.check(eng.lib, eng.lib.spl_ctx_set_rollout_pipeline(eng.ctx, 1))  # auto: one of the shapes above
    for per_step in (False, True):
        assert eng.rollout_kernel_name(per_step=per_step) in forced
