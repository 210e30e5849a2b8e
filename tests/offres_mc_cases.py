"""The table of the entry points of include/pnpadmm_offres_mc.h by what they may do to a running episode, in the classes of
tests/handle_cases.py (imported read-only), the shapes the host and GPU tests share, and the tests that run each entry point (no test in here).

tests/test_offres_mc_host.py requires that this table, the header and `_lib.SIGNATURES_OFFRES_MC` name the same functions with the same
argument counts; tests/test_gpu_offres_mc.py runs the INTRUDER entries between two steps of episodes of the other kinds, and the REPLACES
entries against the other installers in both orders."""
import handle_cases as HC

HEADER = "pnpadmm_offres_mc.h"

# name -> (class, arguments in the header)
ENTRY_POINTS = {
    "pnp_offres_forward_mc": (HC.INTRUDER, 10),
    "pnp_offres_adjoint_mc": (HC.INTRUDER, 11),
    "pnp_set_kspace_offres_mc": (HC.REPLACES, 10),
    "pnp_reset_offres_mc": (HC.REPLACES, 14),
    "pnp_offres_mc_coils": (HC.STATELESS, 1),
    "pnp_offres_mc_cg_residual": (HC.INTRUDER, 3),
    "pnp_offres_mc_normal": (HC.INTRUDER, 5),
    "pnp_acquire_offres_mc": (HC.INTRUDER, 15),
}

# the test of tests/test_gpu_offres_mc.py that makes the call in the role the class names
COVERED_BY = {
    "pnp_offres_forward_mc": "test_the_new_intruders_between_two_steps_of_the_other_kinds_change_nothing",
    "pnp_offres_adjoint_mc": "test_the_new_intruders_between_two_steps_of_the_other_kinds_change_nothing",
    "pnp_acquire_offres_mc": "test_the_new_intruders_between_two_steps_of_the_other_kinds_change_nothing",
    "pnp_set_kspace_offres_mc": "test_installed_last_in_both_orders_the_plan_calls_and_the_getters",
    "pnp_reset_offres_mc": "test_installed_last_in_both_orders_the_plan_calls_and_the_getters",
    "pnp_offres_mc_cg_residual": "test_the_stage_step_composition_cg_dc_stopped_slices_snapshots_and_workspace",
    "pnp_offres_mc_normal": "test_the_stage_step_composition_cg_dc_stopped_slices_snapshots_and_workspace",
}

# The smallest shapes at which the block logic can go wrong.  plan: "linear" or "ls"; sens_n / map_n: 1 (shared) or "n" (per slice)
#          n   h   w   grid       J  trajectory  C  L  plan      sens_n map_n wts
CASES = {
    "A": dict(n=2, h=16, w=16, grid=(32, 32), J=4, kind="radial", C=1, L=1, plan="linear", sens_n=1, map_n=1, wts=False),
    "B": dict(n=3, h=16, w=32, grid=(32, 64), J=6, kind="spiral", C=3, L=3, plan="linear", sens_n=1, map_n="n", wts=True),
    "C": dict(n=2, h=32, w=32, grid=(64, 64), J=6, kind="spiral", C=5, L=9, plan="linear", sens_n="n", map_n=1, wts=False),
    # D: a mixed-radix grid.  Grid sides are sides of the k-space stage (multiples of 16), so 100 x 80 cannot be planned: 160 x 80, both
    # sides of the mixed-radix family
    "D": dict(n=1, h=80, w=64, grid=(160, 80), J=8, kind="rosette", C=9, L=8, plan="ls", sens_n=1, map_n=1, wts=True),
    "E": dict(n=2, h=32, w=32, grid=(64, 64), J=6, kind="spiral", C=2, L=11, plan="ls", sens_n="n", map_n="n", wts=False),
}
COIL_BLOCKS = (1, 2, 4)
SEG_BLOCKS = (1, 3, 8)


def missing(names, table=None):
    """functions of the header that the table does not classify"""
    table = ENTRY_POINTS if table is None else table
    return [n for n in names if n not in table]
