"""The inputs of tests/test_gpu_match_guided_scale.py reach the cases they are built for - asserted on the NumPy restatements and the
C oracle alone, without a GPU: the committed seeds are verified here.  The case builders are the GPU file's own; none of them needs
torch."""
import sys

import numpy as np
import pytest

import test_gpu_match_guided_scale as S
from test_abi_match_mutual import CENTRE, LINE

FORMS = pytest.mark.parametrize("form", [CENTRE, LINE], ids=lambda f: S.FORMS[f])


def test_the_builders_need_no_torch():
    src = open(S.__file__).read()
    top = [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))]
    assert top and not any("torch" in ln for ln in top)
    assert "pytestmark = pytest.mark.gpu" in src


def test_more_pairs_than_one_launch_a_model_per_pair():
    """the seam's three pairs share their frames and differ in their model and in every mode's expected block; a launch-relative model
    index would change at least a quarter of the second launch's good pairs; every table holds rows with 0, 1 and more allowed train
    rows; the mutual tables keep and drop; the keyframe form's blocks under the seam's three models differ too"""
    many = S.Many()
    S.many_checks(many)
    assert set(S.MANY_MODES) == {"guided_k2", "guided_radius", "epi_k2", "epi_radius", "mutual_centre", "mutual_line", "mutual_centre_fallback"}
    kinds = {form: [(m[1], m[2]) for m in S.MANY_MODELS[form]] for form in (CENTRE, LINE)}
    for form in (CENTRE, LINE):                                      # three usable records, the zero model, PAIR_NO_MODEL, hypothesis -1
        assert all(h >= 0 and not f & S.PAIR_NO_MODEL for h, f in kinds[form][:3]) and S.MANY_MODELS[form][3][0] == (0.0,) * 9
        assert kinds[form][4][1] & S.PAIR_NO_MODEL and kinds[form][5][0] == -1


@FORMS
def test_train_indices_beyond_16_bits(form):
    """exact copies above 65 536 allowed and forbidden, equal distances below and above it, allowed rows around the seams of wave
    slices 1 and 7, rows on the list path and on the dense path, and at least 10 reported indices >= 65 536 in every mode"""
    S.wide_wants(S.wide_case(form))


@FORMS
def test_the_long_query_frame(form):
    """every variant - allowed and dropped, forbidden and kept, tied and kept - at every position class of the backward scan"""
    case = S.long_case(form)
    want = S.long_want(case)
    assert {name for name, _, _, _ in case["plan"]} == {"first", "64th", "65th", "last block", "last", "beyond 2^16"}
    assert sorted({w for _, w, _, _ in case["plan"]}) == [1, 7] and len(case["extra"]) == 6
    assert int(want[4].sum()) > 20


@FORMS
def test_the_most_rows_the_keys_hold(form):
    S.limit_want(S.limit_case(form))
    S.limit_mutual_want(S.limit_mutual_case(form))


def test_a_count_the_keys_do_not_hold():
    rows, kps = S.claim_case()
    for form in (CENTRE, LINE):
        for kind, per, radius in (("knn", 2, None), ("radius", 3, 40.5), ("mutual", 1, None)):
            want, pair_rows = S.claim_want(form, kind, per, rows, kps, radius)
            assert [w is None for w in want] == [False, True, kind == "mutual", False]
            if kind == "mutual":
                assert all(0 < w[4].sum() < len(w[4]) for w in want if w is not None)
            else:
                assert all(sum(len(r) for r in w) > 10 for w in want if w is not None)


def test_closed_bounds_at_fractional_centres():
    """at least 90 % of the rows keep their plant (99 % with this model), each of the four bounds in more than 400 rows; an fp32
    division moves enough centres to swap a planted pair in hundreds of rows"""
    case = S.bound_case()
    S.bound_want(case)
    share = case["planted"].mean()
    print("rows that keep their plant: %.4f" % share, file=sys.stderr)
    h = np.asarray(S.BOUND_H, np.float64)
    x, y = case["kq"]["x"].astype(np.float64), case["kq"]["y"].astype(np.float64)
    z, u, v = (h[6] * x + h[7] * y) + h[8], (h[0] * x + h[1] * y) + h[2], (h[3] * x + h[4] * y) + h[5]
    c32 = np.where(case["bound"] < 2, u.astype(np.float32) / z.astype(np.float32), v.astype(np.float32) / z.astype(np.float32))
    c64 = np.where(case["bound"] < 2, case["centres"][0], case["centres"][1])
    assert ((c32 != c64) & case["planted"]).sum() > 200


def test_closed_bounds_of_the_band():
    S.band_want(S.band_case())
