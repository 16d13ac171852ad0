"""The per-Gaussian forward kernels after their loads were rescheduled (one trip to memory per wave): every output byte
is the one the build before the change wrote (tests/golden/G14_preprocess_getter_parent*.npz, written by
tests/golden/make_load_order_golden.py on that build).  Not a tolerance: np.array_equal on every array."""
import functools
import os

import numpy as np
import pytest

import load_order_cases as LC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden(fn):
    with np.load(os.path.join(LC.GOLDEN_DIR, fn)) as z:
        return {k: z[k] for k in z.files}


def _same(name, got, fn="G14_preprocess_getter_parent.npz"):
    gold = _golden(fn)
    keys = sorted(k.split("/", 1)[1] for k in gold if k.startswith(name + "/"))
    assert keys == sorted(got), f"{name}: stored arrays {keys} != computed {sorted(got)}"
    bad = []
    for k in keys:
        a, b = got[k], gold[f"{name}/{k}"]
        if not (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)):
            n = int((a.reshape(-1) != b.reshape(-1)).sum()) if a.shape == b.shape else -1
            bad.append(f"{k}: {n} of {b.size} elements differ (dtype {a.dtype}/{b.dtype}, shape {a.shape}/{b.shape})")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(LC.PROJECTION_CASES))
def test_projection_same_bits_as_before(name):
    """P = 1, 63, 65, 257, 1000 (partial last wave, more than one workgroup) at SH degree 3; rows of 3, 12, 27 and 48 floats
    (both paths of the SH row copy); precomputed colours without SH rows; precomputed covariances without scales/rotations."""
    _same(name, LC.run_projection(name))


@pytest.mark.parametrize("name", list(LC.CULLED_CASES))
def test_fully_culled_wave_between_visible_ones(name):
    got = LC.run_culled(name)
    _, rows = LC.culled_scene(name)
    # culled rows: zero record, radius 0, no tile; the block sums (hence D) count the visible rows only
    for k in ("depth", "xy", "conic_opacity", "rgb", "normal", "tiles_touched", "radii"):
        assert not got[k][rows].any(), f"{name}: {k} of a culled row is not zero"
    assert int(got["D"][0]) == int(got["tiles_touched"].astype(np.int64).sum()) == got["keys_sorted"].shape[0]
    assert (got["radii"][rows.stop:] > 0).any(), "the rows after the culled wave are visible"
    assert rows.start == 0 or (got["radii"][:rows.start] > 0).any(), "the rows before the culled wave are visible"
    _same(name, got)


@pytest.mark.parametrize("name", list(LC.GETTER_CASES))
def test_dynamic_getter_same_bits_as_before(name):
    """P = 1, 1023, 1025, 2500 x Tu = 1, 7, 100 with random birth indices (one workgroup short of full, one row into the
    second, three workgroups; a table of one row, of less than one trip, of three trips), and one call without upstream
    gradients: the four forward outputs, the five backward gradients and the birth-sorted copy."""
    _same(name, LC.run_getter(name), LC.getter_file(name))
