"""
pipeline.step_outputs, the table of the optional per-group outputs of a step (no GPU): the records it returns, their
fixed order, and that the arguments pipeline.Workspace rejects are rejected here with the same exception types.
"""
import numpy as np
import pytest

from tda_eeg_audio_amd import pipeline, utils
from tda_eeg_audio_amd._lib import TdaError

GRID, LEVELS = np.linspace(0.0, 1.5, 16), 2
IMAGES = (np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 6), 0.1, 1)        # 4 x 5 pixels
DIRS = utils.default_directions(4)
ALL = dict(correlations=True, bottleneck=True, landscapes=(GRID, LEVELS), images=IMAGES, sliced=DIRS)
# all eleven: the five above and the six added since, in the order of the table
EVERY = dict(ALL, wasserstein_q=(2, "l2"), frechet=(8, 4), kernel_distance=("pss", 0.1), fisher=0.1, sublevel=True,
             phase_locking="euclidean")


def test_everything_off_is_an_empty_table():
    assert pipeline.step_outputs() == []
    assert pipeline.step_outputs(correlations=False, bottleneck=False, landscapes=None, images=None, sliced=None) == []


@pytest.mark.parametrize("option,name,shape", [
    ("correlations", "corr", (10,)),
    ("bottleneck", "bott", (2,)),
    ("landscapes", "land", (3, 3, 16)),
    ("images", "img", (3, 5, 4)),
    ("sliced", "slc", (2,)),
    ("wasserstein_q", "wq", (2,)),
    ("frechet", "fm", (3, 10, 2)),
    ("kernel_distance", "kd", (2,)),
    ("fisher", "pf", (2,)),
    ("sublevel", "sl", (22,)),
    ("phase_locking", "pl", (24,)),
])
def test_each_output_alone(option, name, shape):
    (o,) = pipeline.step_outputs(**{option: EVERY[option]})
    assert (o.name, o.shape) == (name, shape)


def test_validated_parameters():
    par = {o.name: o.params for o in pipeline.step_outputs(**ALL)}
    grid, levels = par["land"]
    assert grid.dtype == np.float64 and np.array_equal(grid, GRID) and levels == LEVELS and isinstance(levels, int)
    xe, ye, sigma, power = par["img"]
    assert np.array_equal(xe, IMAGES[0]) and np.array_equal(ye, IMAGES[1]) and (sigma, power) == (0.1, 1)
    assert par["slc"].dtype == np.float64 and par["slc"].flags.c_contiguous and np.array_equal(par["slc"], DIRS)


def test_all_on_in_the_fixed_order():
    assert [o.name for o in pipeline.step_outputs(**ALL)] == ["corr", "bott", "land", "img", "slc"]
    assert [o.shape for o in pipeline.step_outputs(**ALL)] == [(pipeline.CORR_COLS,), (pipeline.BOTT_COLS,), (pipeline.LAND_SETS, 3, 16),
                                                               (pipeline.IMG_SETS, 5, 4), (pipeline.SLC_COLS,)]
    # the order is the table's, not the caller's
    assert [o.name for o in pipeline.step_outputs(sliced=DIRS, bottleneck=True)] == ["bott", "slc"]


def test_all_eleven_on_in_the_fixed_order():
    outs = pipeline.step_outputs(**EVERY)
    assert [o.name for o in outs] == ["corr", "bott", "land", "img", "slc", "wq", "fm", "kd", "pf", "sl", "pl"]
    assert [o.shape for o in outs] == [(10,), (2,), (3, 3, 16), (3, 5, 4), (2,), (2,), (3, 10, 2), (2,), (2,), (22,), (24,)]
    assert [o.name for o in pipeline.step_outputs(**dict(reversed(list(EVERY.items()))))] == [o.name for o in outs]


def test_table_order_is_the_positional_order():
    import inspect
    keywords = [rec.keyword for rec in pipeline.OUTPUTS]
    assert keywords == list(inspect.signature(pipeline.step_outputs).parameters) == list(EVERY)
    assert [rec.name for rec in pipeline.OUTPUTS] == [o.name for o in pipeline.step_outputs(*(EVERY[k] for k in keywords))]
    for i, rec in enumerate(pipeline.OUTPUTS):                     # every keyword alone at its own position
        args = [None] * i + [EVERY[rec.keyword]]
        assert [o.name for o in pipeline.step_outputs(*args)] == [rec.name]


def test_launch_order_is_not_the_table_order():
    """The stage names of a step with everything on, between `finish` and `reduce`, from the records and LAUNCH_ORDER."""
    stages = [s for name in pipeline.LAUNCH_ORDER
              for s in (("wasserstein_h0", "wasserstein_h1") if name is None else pipeline.OUTPUT_BY_NAME[name].stages)]
    assert stages == ["temporal_corr", "landscape", "image", "wasserstein_h0", "wasserstein_h1", "bottleneck_h0", "bottleneck_h1",
                      "sliced_h0", "sliced_h1", "wasserstein_q_h0", "wasserstein_q_h1", "kernel_distance_h0",
                      "kernel_distance_h1", "fisher_h0", "fisher_h1", "frechet", "sublevel", "phase_locking"]
    assert sorted(n for n in pipeline.LAUNCH_ORDER if n is not None) == sorted(rec.name for rec in pipeline.OUTPUTS)
    assert [rec.name for rec in pipeline.OUTPUTS if rec.set_stage is not None] == ["land", "img", "fm"]      # run_features_step


def test_unknown_keyword_is_a_type_error():
    with pytest.raises(TypeError):
        pipeline.step_outputs(nonsense=1)
    with pytest.raises(TypeError):
        pipeline.step_outputs(*([None] * 12))


@pytest.mark.parametrize("kw,exc", [
    (dict(landscapes=(GRID, 0)), ValueError),
    (dict(landscapes=(GRID, 9)), ValueError),
    (dict(landscapes=(np.zeros(0), LEVELS)), ValueError),
    (dict(landscapes=(np.linspace(0.0, 1.0, 257), LEVELS)), ValueError),
    (dict(images=(np.array([0.0, 0.5, 0.25, 1.0]), IMAGES[1], 0.1, 1)), ValueError),
    (dict(images=(IMAGES[0], IMAGES[1], 0.0, 1)), ValueError),
    (dict(sliced=np.zeros((2, 3))), TdaError),
    (dict(sliced=[[np.nan, 1.0]]), TdaError),
])
def test_invalid_arguments(kw, exc):
    with pytest.raises(exc):
        pipeline.step_outputs(**kw)
