"""The table of the entry points of include/pnpadmm_offres.h by what they may do to a running episode, in the classes of
tests/handle_cases.py (imported read-only), and the tests that run each of them (no test in here).

tests/test_offres_host.py requires that this table, the header and `_lib.SIGNATURES_OFFRES` name the same functions with the same argument
counts; tests/test_gpu_offres.py runs the INTRUDER entries between two steps of episodes of every stage kind, and the REPLACES entries
against the other installers in both orders."""
import handle_cases as HC

HEADER = "pnpadmm_offres.h"

# name -> (class, arguments in the header)
ENTRY_POINTS = {
    "pnp_offres_plan": (HC.REPLACES, 4),
    "pnp_offres_segments": (HC.STATELESS, 1),
    "pnp_offres_maps": (HC.INTRUDER, 5),
    "pnp_offres_forward": (HC.INTRUDER, 7),
    "pnp_offres_adjoint": (HC.INTRUDER, 8),
    "pnp_set_kspace_offres": (HC.REPLACES, 7),
    "pnp_reset_offres": (HC.REPLACES, 11),
    "pnp_offres_live": (HC.STATELESS, 1),
    "pnp_offres_cg_residual": (HC.INTRUDER, 3),
    "pnp_offres_normal": (HC.INTRUDER, 5),
    "pnp_acquire_offres": (HC.INTRUDER, 12),
}

# the test of tests/test_gpu_offres.py that makes the call in the role the class names
COVERED_BY = {
    "pnp_offres_plan": "test_the_new_stage_against_the_other_stages_in_both_orders_and_both_plan_calls",
    "pnp_set_kspace_offres": "test_the_new_stage_against_the_other_stages_in_both_orders_and_both_plan_calls",
    "pnp_reset_offres": "test_the_new_stage_against_the_other_stages_in_both_orders_and_both_plan_calls",
    "pnp_offres_maps": "test_the_intruders_between_two_steps_of_an_episode_of_every_kind_change_nothing",
    "pnp_offres_forward": "test_the_intruders_between_two_steps_of_an_episode_of_every_kind_change_nothing",
    "pnp_offres_adjoint": "test_the_intruders_between_two_steps_of_an_episode_of_every_kind_change_nothing",
    "pnp_acquire_offres": "test_the_intruders_between_two_steps_of_an_episode_of_every_kind_change_nothing",
    "pnp_offres_cg_residual": "test_the_stage_step_composition_cg_dc_stopped_slices_and_snapshots",
    "pnp_offres_normal": "test_the_stage_step_composition_cg_dc_stopped_slices_and_snapshots",
}


def missing(names, table=None):
    """functions of the header that the table does not classify"""
    table = ENTRY_POINTS if table is None else table
    return [n for n in names if n not in table]
