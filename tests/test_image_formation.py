"""The CPU oracle's image formation against closed forms (tests/image_ref.py) on the scenes of tests/image_cases.py: the
pixel-to-ray mapping (row order, the half-pixel, aspect, vertical vfov), the box and triangle filters at the radius a render
uses, the thin lens (aperture as a diameter, the disc, the offset's sign), the shutter draw, the 256-pixel tile domain and
the adaptive stopping rule, against values that do not come from the oracle's author. The parity suite compares the
device with the oracle bit for bit; this is what says the oracle (and so the device) puts the right value in the right
pixel. tests/test_gpu_image_formation.py runs the same cases on the device.

Per case: frames 0..3 at 256 spp, the mean image against the truth for EVERY pixel and channel,
    |mean - truth| <= (5 sqrt(e) sqrt(p (1 - p) / 1024) + allowance) * |card - backdrop|,
p the true coverage, sqrt(e) Owen's bound on a scrambled net's variance against Monte Carlo's, the allowance from
image_cases.MEASURED (at most 2e-3); a pixel with p = 0 or 1 equals its colour exactly; and the same bound on every row
sum and column sum (image_cases.violations)."""
import numpy as np
import pytest

import image_cases as ic
import image_ref as ir

CASES = {c.name: c for c in ic.cases()}
_means, _samples = {}, {}


def mean_image(name):
    if name not in _means:
        _means[name] = ic.mean_image(ic.oracle_render, CASES[name])
    return _means[name]


def stop_samples(luminance):
    """(case, [20, 24, 64, 3] sample colours of the oracle), rendered once for the five rules."""
    if luminance not in _samples:
        case = ic.stop_case(luminance)
        _samples[luminance] = (case, ic.oracle_samples(case, ic.STOP_SPP))
    return _samples[luminance]


# ---------------------------------------------------------------- the truth itself ----------------------------------------------------------------
def test_the_closed_forms_pass_their_own_checks():
    assert ir.self_test()


def test_the_cases_are_the_ones_the_bound_was_measured_for():
    assert set(ic.MEASURED) == set(CASES)
    for name, c in CASES.items():
        assert 0.0 <= c.allowance() <= 2e-3, name
    assert CASES["lens_flat_field"].allowance() == 0.0


def test_the_cases_say_what_they_are_meant_to():
    slanted = CASES["pinhole_slanted"].coverage()
    assert np.array_equal(CASES["lens_in_focus"].coverage(), slanted)  # d = f: the lens does not show
    # no row and no column of the slanted case equals its mirror image, nor the transposed frame's: a flip or a transpose shows
    assert not np.any(np.all(slanted == slanted[::-1], axis=1)) and not np.any(np.all(slanted == slanted[:, ::-1], axis=0))
    # the edge passes no pixel corner within 1e-3 pixels: no pixel's being on the edge hangs on rounding
    nx, ny, c = ic.SLANTED
    i, j = np.meshgrid(np.arange(ic.W + 1), np.arange(ic.H + 1))
    assert np.abs(nx * i + ny * j - c).min() > 1e-3
    # the blur of the lens cases spans more than a pixel on either side of the focus plane, mirrored behind it
    near = ir.lens_blur(CASES["lens_defocus_diagonal"].cam, ic.W, ic.H, 0.6 * ir.camera_frame(CASES["lens_defocus_diagonal"].cam)["focus"])
    far = ir.lens_blur(CASES["lens_defocus_behind"].cam, ic.W, ic.H, 1.5 * ir.camera_frame(CASES["lens_defocus_behind"].cam)["focus"])
    assert near > 1.5 and far < -0.75
    # the strip's edge lies in the second 256-pixel tile domain
    assert np.argwhere((CASES["wide_strip"].coverage() > 0) & (CASES["wide_strip"].coverage() < 1))[:, 1].tolist() == [257, 257]


# ---------------------------------------------------------------- the oracle against it ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_the_closed_form_in_every_pixel(name):
    case = CASES[name]
    mean = mean_image(name)
    bad = ic.violations(case, mean, ic.FRAMES * ic.SPP, case.allowance())
    print("%s: largest deviation %.2e of the contrast, allowance %.1e, %d violations" % (name, ic.deviation(case, mean), case.allowance(), len(bad)))
    assert not bad, (name, len(bad), bad[:4])


def test_a_flat_field_is_flat_under_any_lens_and_filter():
    case = CASES["lens_flat_field"]
    for f in range(ic.FRAMES):
        img = ic.oracle_render(case.build(f), ic.SPP)
        assert np.all(img == ic.BACKDROP.astype(np.float32)), f


# ---------------------------------------------------------------- the stopping rule ----------------------------------------------------------------
@pytest.mark.parametrize("luminance", [None, 3e-5], ids=["bright", "under-the-floor"])
@pytest.mark.parametrize("min_spp,threshold", ic.STOP_RULES)
def test_oracle_stops_where_the_rule_says(luminance, min_spp, threshold):
    """render_pixel's adaptive stop (tracer.rs:609-617) on a two-valued pixel: the count of every pixel is
    image_ref.stop_count of the sequence of its samples, and the pixel is the float32 sum of that many sample colours, in
    order, over the count."""
    case, samples = stop_samples(luminance)
    want, lit = ic.expected_counts(case, samples, min_spp, threshold)
    counts, img = ic.oracle_adaptive(case, ic.STOP_SPP, min_spp, threshold)
    assert np.array_equal(counts, want), (np.argwhere(counts != want)[:4], counts[counts != want][:4], want[counts != want][:4])
    ic.check_stop_shape(counts, lit, min_spp, threshold, bright=luminance is None)
    assert np.array_equal(img.view(np.uint32), ic.sequential_mean(samples, counts).view(np.uint32))


def test_the_floor_changes_the_counts():
    """Under the 1e-4 floor the rule stops pixels the bright card keeps sampling: the second variant tests the floor."""
    (bright, s_b), (dim, s_d) = stop_samples(None), stop_samples(3e-5)
    a, lit_a = ic.expected_counts(bright, s_b, 1, 0.05)
    b, lit_b = ic.expected_counts(dim, s_d, 1, 0.05)
    assert np.array_equal(lit_a, lit_b) and np.any(b < a) and np.all(b <= a)
