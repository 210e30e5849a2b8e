"""The table of the entry points of include/pnpadmm_offres_tz.h by what they may do to a running episode, in the classes of
tests/handle_cases.py (imported read-only), the shapes the host and GPU tests share, and the tests that run each entry point (no test in here).

tests/test_offres_tz_host.py requires that this table, the header and `_lib.SIGNATURES_OFFRES_TZ` name the same functions with the same
argument counts; tests/test_gpu_offres_tz.py runs the INTRUDER entries between two steps of episodes of the other kinds, and the REPLACES
entries against the other installers in both orders."""
import handle_cases as HC

HEADER = "pnpadmm_offres_tz.h"

# name -> (class, arguments in the header)
ENTRY_POINTS = {
    "pnp_offres_tz_plan": (HC.REPLACES, 4),
    "pnp_offres_tz_planned": (HC.STATELESS, 1),
    "pnp_offres_tz_live": (HC.STATELESS, 1),
    "pnp_offres_tz_spectra": (HC.STATELESS, 1),
    "pnp_offres_tz_spectrum": (HC.INTRUDER, 3),
    "pnp_offres_tz_apply": (HC.INTRUDER, 7),
    "pnp_offres_tz_apply_mc": (HC.INTRUDER, 10),
    "pnp_set_kspace_offres_tz": (HC.REPLACES, 6),
    "pnp_reset_offres_tz": (HC.REPLACES, 10),
    "pnp_set_kspace_offres_mc_tz": (HC.REPLACES, 9),
    "pnp_reset_offres_mc_tz": (HC.REPLACES, 13),
}

# the test of tests/test_gpu_offres_tz.py that makes the call in the role the class names
COVERED_BY = {
    "pnp_offres_tz_plan": "test_installed_last_in_both_orders_and_the_plan_calls",
    "pnp_offres_tz_spectrum": "test_the_intruders_between_two_steps_of_the_other_kinds_change_nothing",
    "pnp_offres_tz_apply": "test_the_intruders_between_two_steps_of_the_other_kinds_change_nothing",
    "pnp_offres_tz_apply_mc": "test_the_intruders_between_two_steps_of_the_other_kinds_change_nothing",
    "pnp_set_kspace_offres_tz": "test_installed_last_in_both_orders_and_the_plan_calls",
    "pnp_reset_offres_tz": "test_installed_last_in_both_orders_and_the_plan_calls",
    "pnp_set_kspace_offres_mc_tz": "test_installed_last_in_both_orders_and_the_plan_calls",
    "pnp_reset_offres_mc_tz": "test_installed_last_in_both_orders_and_the_plan_calls",
}

# The smallest shapes at which each piece can go wrong; the rows are read by tests/offres_mc_ref.py's case_* helpers.  plan: "linear" or "ls";
# sens_n / map_n: 1 (shared) or "n" (per slice); dense: the dense operator A^H W A is small enough to be the reference
#          n   h   w   grid       J  trajectory  C  L  plan      sens_n map_n wts
CASES = {
    "A": dict(n=2, h=16, w=16, grid=(32, 32), J=4, kind="radial", C=1, L=1, plan="linear", sens_n=1, map_n=1, wts=False, dense=True),
    "B": dict(n=3, h=16, w=32, grid=(32, 64), J=6, kind="spiral", C=1, L=3, plan="linear", sens_n=1, map_n="n", wts=True, dense=True),
    "C": dict(n=2, h=32, w=32, grid=(64, 64), J=6, kind="spiral", C=1, L=9, plan="linear", sens_n=1, map_n=1, wts=False, dense=True),
    # D: a mixed-radix padded grid (160 x 128): the composed form only
    "D": dict(n=1, h=80, w=64, grid=(160, 80), J=8, kind="rosette", C=1, L=8, plan="ls", sens_n=1, map_n=1, wts=True, dense=True),
    "E": dict(n=2, h=32, w=32, grid=(64, 64), J=6, kind="spiral", C=3, L=11, plan="ls", sens_n="n", map_n=1, wts=False, dense=True),
    # F, G: 2H = 256 and 512, the register-resident line transforms of the column passes; the dense operator is too large, the reference
    # is the float64 FFT form
    "F": dict(n=1, h=128, w=128, grid=(256, 256), J=6, kind="spiral", C=1, L=2, plan="linear", sens_n=1, map_n=1, wts=False, dense=False),
    "G": dict(n=1, h=256, w=256, grid=(512, 512), J=6, kind="spiral", C=1, L=2, plan="linear", sens_n=1, map_n=1, wts=False, dense=False),
}
HOST_CASES = ("A", "B", "C", "E")        # the float64 identities of tests/test_offres_tz_host.py (16 x 16, 16 x 32, 32 x 32; L = 1, 3, 9 linear, 11 ls)
SLICE_BLOCKS = (1,)                      # PNP_OFFRES_TZ_SLICE_BLOCK values run beside the default
COIL_BLOCKS = (1, 2)                     # PNP_OFFRES_MC_COIL_BLOCK values of the multi-coil case


def missing(names, table=None):
    """functions of the header that the table does not classify"""
    table = ENTRY_POINTS if table is None else table
    return [n for n in names if n not in table]
