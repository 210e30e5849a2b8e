"""The table of the entry points of include/pnpadmm_ncsense.h by what they may do to a running episode, in the classes of
tests/handle_cases.py (imported read-only), and the tests that run each of them (no test in here).

tests/test_ncsense_host.py requires that this table, the header and `_lib.SIGNATURES_NCSENSE` name the same functions with the same
argument counts; tests/test_gpu_ncsense.py runs the INTRUDER entries between two steps of episodes of every kind, and each REPLACES entry
followed by a re-install."""
import handle_cases as HC

HEADER = "pnpadmm_ncsense.h"

# name -> (class, arguments in the header)
ENTRY_POINTS = {
    "pnp_set_kspace_ncsense": (HC.REPLACES, 8),
    "pnp_reset_ncsense": (HC.REPLACES, 12),
    "pnp_ncsense_coils": (HC.STATELESS, 1),
    "pnp_nufft_forward_mc": (HC.INTRUDER, 8),
    "pnp_nufft_adjoint_mc": (HC.INTRUDER, 9),
    "pnp_ncsense_cg_residual": (HC.INTRUDER, 3),
    "pnp_ncsense_normal": (HC.INTRUDER, 5),
    "pnp_acquire_ncsense": (HC.INTRUDER, 13),
}

# the test of tests/test_gpu_ncsense.py that makes the call in the role the class names
COVERED_BY = {
    "pnp_set_kspace_ncsense": "test_every_installer_followed_by_a_reinstall_restores_the_bits",
    "pnp_reset_ncsense": "test_every_installer_followed_by_a_reinstall_restores_the_bits",
    "pnp_nufft_forward_mc": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_nufft_adjoint_mc": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_acquire_ncsense": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_ncsense_cg_residual": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_ncsense_normal": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
}


def missing(names, table=None):
    """functions of the header that the table does not classify"""
    table = ENTRY_POINTS if table is None else table
    return [n for n in names if n not in table]
