"""The table of the entry points of include/pnpadmm_dcf.h by what they may do to a running episode, in the classes of
tests/handle_cases.py (imported read-only), and the tests that run each of them (no test in here).

tests/test_dcf_host.py requires that this table, the header and `_lib.SIGNATURES_DCF` name the same functions with the same argument
counts; tests/test_gpu_dcf.py runs both between two steps of episodes of every non-Cartesian kind."""
import handle_cases as HC

HEADER = "pnpadmm_dcf.h"

# name -> (class, arguments in the header)
ENTRY_POINTS = {
    "pnp_nufft_psi": (HC.INTRUDER, 4),
    "pnp_nufft_dcf": (HC.INTRUDER, 7),
}

# the test of tests/test_gpu_dcf.py that makes the call in the role the class names
COVERED_BY = {
    "pnp_nufft_psi": "test_the_two_calls_between_two_steps_of_an_episode_change_nothing",
    "pnp_nufft_dcf": "test_the_two_calls_between_two_steps_of_an_episode_change_nothing",
}


def missing(names, table=None):
    """functions of the header that the table does not classify"""
    table = ENTRY_POINTS if table is None else table
    return [n for n in names if n not in table]
