"""The table of the entry points of include/pnpadmm_toeplitz.h by what they may do to a running episode, in the classes of
tests/handle_cases.py (imported read-only), and the tests that run each of them (no test in here).

tests/test_toeplitz_host.py requires that this table, the header and `_lib.SIGNATURES_TOEPLITZ` name the same functions with the same
argument counts; tests/test_gpu_toeplitz.py runs the INTRUDER entries between two steps of episodes of every kind, and each REPLACES entry
followed by a re-install."""
import handle_cases as HC

HEADER = "pnpadmm_toeplitz.h"

# name -> (class, arguments in the header)
ENTRY_POINTS = {
    "pnp_toeplitz_plan": (HC.REPLACES, 4),          # replaces the spectrum; drops a live Toeplitz stage's constants
    "pnp_toeplitz_planned": (HC.STATELESS, 1),
    "pnp_toeplitz_live": (HC.STATELESS, 1),
    "pnp_toeplitz_spectrum": (HC.INTRUDER, 3),
    "pnp_toeplitz_apply": (HC.INTRUDER, 5),
    "pnp_toeplitz_apply_mc": (HC.INTRUDER, 8),
    "pnp_set_kspace_nc_tz": (HC.REPLACES, 4),
    "pnp_reset_nc_tz": (HC.REPLACES, 8),
    "pnp_set_kspace_ncsense_tz": (HC.REPLACES, 7),
    "pnp_reset_ncsense_tz": (HC.REPLACES, 11),
}

# the test of tests/test_gpu_toeplitz.py that makes the call in the role the class names
COVERED_BY = {
    "pnp_toeplitz_plan": "test_replanning_drops_what_the_header_says_it_drops",
    "pnp_toeplitz_spectrum": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_toeplitz_apply": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_toeplitz_apply_mc": "test_the_new_intruders_between_two_steps_of_an_episode_change_nothing",
    "pnp_set_kspace_nc_tz": "test_every_tz_installer_followed_by_a_reinstall_restores_the_bits",
    "pnp_reset_nc_tz": "test_every_tz_installer_followed_by_a_reinstall_restores_the_bits",
    "pnp_set_kspace_ncsense_tz": "test_every_tz_installer_followed_by_a_reinstall_restores_the_bits",
    "pnp_reset_ncsense_tz": "test_every_tz_installer_followed_by_a_reinstall_restores_the_bits",
}


def missing(names, table=None):
    """functions of the header that the table does not classify"""
    table = ENTRY_POINTS if table is None else table
    return [n for n in names if n not in table]
