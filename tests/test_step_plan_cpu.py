"""Host side of the one-call plan (models/step_plan.py): what needs no device -- the transitions of ImageFreshness, the one owner
of the question whether a plan's weight images still follow the parameters."""
import pytest
import torch

KEY = ("gen", 13, (1, 0), False)
OTHER = ("gen", 13, (1, 0), True)


@pytest.fixture()
def eng():
    import gnn_tableextraction_amd as gte
    from gnn_tableextraction_amd.models.engine import FusedGcnSageStep
    torch.manual_seed(0)
    e = FusedGcnSageStep(gte.GcnSAGE(13, 64, 9, 3, torch.nn.functional.relu, 0))
    e.wimg_in_fold = True                             # (whatever GTE_WIMG_IN_FOLD says in this environment)
    return e


def test_images_are_fresh_for_the_key_that_was_written_until_the_parameters_move(eng):
    im = eng._plan.images
    assert eng._wimg_sig is None and not im.fresh(KEY, False)
    im.wrote(KEY, False)
    assert im.fresh(KEY, False) and eng._wimg_sig is not None
    assert not im.fresh(OTHER, False)                 # a plan of another layout keeps its own images
    im.wrote(KEY, False)                              # (... whichever key was asked about last)
    assert im.fresh(KEY, False) and not im.fresh(OTHER, False)
    assert not im.fresh(KEY, True)                    # nothing is current while capturing
    with torch.no_grad():
        next(eng.model.parameters()).mul_(1.0)        # an in-place change through torch moves the version counter
    assert not im.fresh(KEY, False)
    im.wrote(KEY, False)
    with torch.no_grad():
        eng.flat_param.mul_(1.0)                      # ... and so does one of the flat buffer the parameters are views of
    assert not im.fresh(KEY, False)


def test_begin_stale_capture_and_the_switch_leave_the_images_stale(eng):
    im = eng._plan.images
    for make_stale in (im.begin, im.stale, eng.invalidate_weight_images):
        im.wrote(KEY, False)
        assert im.fresh(KEY, False)
        make_stale()
        assert not im.fresh(KEY, False) and eng._wimg_sig is None
    im.wrote(KEY, True)                               # a captured launch has not run: it marks nothing
    assert not im.fresh(KEY, False) and eng._wimg_sig is None
    im.wrote(KEY, False)
    eng.wimg_in_fold = False                          # GTE_WIMG_IN_FOLD=0: every forward converts
    assert not im.fresh(KEY, False)


def test_what_a_step_leaves_for_the_optimiser_is_taken_once_or_dropped(eng):
    im = eng._plan.images
    keep = object()
    assert im.take_for_optimiser() is None
    im.wrote(KEY, False)
    im.leave_for_optimiser(1234, 6, KEY, keep)
    assert im.fresh(KEY, False)                       # (leaving changes nothing: a step without an optimiser launch stays fresh)
    assert im.take_for_optimiser() == (1234, 6, KEY, keep)
    assert not im.fresh(KEY, False)                   # the optimiser launch that took them changes the parameters
    assert im.take_for_optimiser() is None            # exactly once
    for drop in (im.stale, im.begin):
        im.leave_for_optimiser(1234, 6, KEY, keep)
        drop()
        assert im.take_for_optimiser() is None


def test_the_engine_reads_the_signature_and_cannot_assign_it(eng):
    with pytest.raises(AttributeError):
        eng._wimg_sig = None
    assert not hasattr(eng, "_last_wimg") and not hasattr(eng, "_plan_images_stale")
