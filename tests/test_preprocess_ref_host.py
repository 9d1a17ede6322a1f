"""Host check of the preprocess checker (tests/exact_preprocess.py; no GPU): the float32 restatement of k_preprocess224 is held to
float64 ATen bicubic under the bound derived in that module, the float64 evaluation of the same formula agrees with ATen to 1e-13
(the formula is right; only rounding separates the two), the bound rejects every listed mutant of the restatement, and the case
table covers every named class.  Prints the worst err/bound per case.

Worst ratio of the unmutated restatement over all cases, as printed by test_restatement_under_bound: 0.080 (300 x 320 pad; the
16-pixel cases 0.002 .. 0.033).  The bound is a worst case over every rounding of the coordinate and of the Horner forms, which
do not all fall the same way; the mutants miss it by factors of 800 and more."""
import numpy as np
import pytest

import exact_preprocess as E

ALL = E.CASES224 + E.HOST_EXTRA


def _args(c):
    return (c["pad"][0], c["pad"][1], c["RH"], c["RW"], c["top"], c["left"], c["size"])


def _first_images(c):
    """the distinct image sizes of a case (the batch-split case repeats two)"""
    seen, out = set(), []
    for hw, img in zip(c["images"], E.case_images(c)):
        if hw not in seen:
            seen.add(hw)
            out.append(img)
    return out


def _ratios(c, mutant=None):
    worst = 0.0
    for img in _first_images(c):
        ref = E.preprocess224_f64(img, *_args(c), E.CLIP_MEAN, E.CLIP_STD)
        got = E.preprocess224_f32(img, *_args(c), E.CLIP_MEAN, E.CLIP_STD, mutant=mutant)
        bound = E.bound224(img, *_args(c), E.CLIP_STD, ref)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / bound).max()))
    return worst


def test_case_table_covers_every_class():
    E.check_case_table()


def test_formula_in_float64_is_aten_bicubic():
    for c in ALL:
        for img in _first_images(c):
            ref = E.preprocess224_f64(img, *_args(c), E.CLIP_MEAN, E.CLIP_STD)
            got = E.preprocess224_formula(img, *_args(c), E.CLIP_MEAN, E.CLIP_STD, ft=np.float64)
            assert float(np.abs(got - ref).max()) <= 1e-13 * (1 + float(np.abs(ref).max())), c["name"]


def test_restatement_under_bound(capsys):
    lines, worst = ["", "preprocess224 f32 restatement vs float64 ATen, worst err/bound per case:"], 0.0
    for c in ALL:
        r = _ratios(c)
        worst = max(worst, r)
        lines.append(f"  {c['name']:20s} pad {c['pad'][0]:3d}x{c['pad'][1]:<3d} size {c['size']:3d}   {r:.3f}")
    lines.append(f"  worst                                      {worst:.3f}")
    with capsys.disabled():
        print("\n".join(lines))
    assert worst < 1.0


# a mutant shows only where the geometry makes it differ: top != 0 for the dropped offset, a non-square batch for the swap, an image
# smaller than its pad for the clamp
MUTANT_CASES = {"A=-0.5": ["portrait", "upscale", "real_size"], "top dropped": ["portrait", "real_size", "host_tall"],
                "sx/sy swapped": ["short_in_tall_pad", "host_300"], "clamp at h-1": ["short_in_tall_pad", "identity"],
                "half-pixel shift": ["portrait", "landscape", "upscale"]}


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_bound_rejects_mutant(mutant, capsys):
    by = {c["name"]: c for c in ALL}
    assert set(MUTANT_CASES) == set(E.MUTANTS)
    rs = {n: _ratios(by[n], mutant) for n in MUTANT_CASES[mutant]}
    with capsys.disabled():
        print(f"\n  mutant {mutant:18s} err/bound " + ", ".join(f"{n} {r:.1f}" for n, r in rs.items()))
    assert all(r > 1.0 for r in rs.values()), rs


def test_preprocess_restatement_against_float64():
    """the full-resolution kernel's expression: two IEEE divisions and one subtraction, each within u of the float64 value"""
    img = E.seeded_image(7, 9, 3)
    for mean, std, div in ((E.CLIP_MEAN, E.CLIP_STD, True), (E.STOCK_MEAN, E.STOCK_STD, False)):
        got = E.preprocess_f32(img, 8, 12, mean, std, div).astype(np.float64)
        m, s = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
        v = img.astype(np.float64).transpose(1, 2, 0) / (255.0 if div else 1.0)
        ref = np.zeros((8, 12, 3))
        ref[:7, :9] = (v - m) / s
        bound = E.U * (2 * np.abs(ref[:7, :9]) + 2 * np.abs(v) / s) + 1e-12     # x/div and the subtraction, then the division
        assert (np.abs(got - ref)[:7, :9] <= bound).all()
        assert (got[7:] == 0).all() and (got[:, 9:] == 0).all()
