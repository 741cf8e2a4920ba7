"""Volume regions without a GPU: the device source of kernels/volume.hip.h compiled for the host (tests/host_shade/
volume_host.cpp) against the float32 numpy restatement of volume.rs (tests/volume_ref.py) bit for bit, the host-built
image against the restatement's derived records, the reference's own unit tests (volume.rs:561-799) and its two USD
tests (usd_scene.rs:192-271) ported with their tolerances and counts, the importer's gating, every refusal of
crt_volumes_new, the argument checks of the batched entry points, the step limit, and a stand-alone sanitizer program.

The statistical unit tests use the project's random stream (the reference's openqmc::pcg::Rng is not in its tree), so
they re-check the statistics, not bits."""
import ctypes as C
import os
import subprocess
import warnings

import numpy as np
import pytest

import volume_cases as vc
import volume_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
f32, u32 = np.float32, np.uint32
N = 2000  # segments per aggregate: the hand-made ones, then seeded random ones
EVENT_FIELDS = ["p", "t", "weight", "kind", "emitted", "n_lobes", "dir", "pdf", "lobes", "status"]
CENTRES = {"scaled_grey": (5, 0, 0), "smoke": (0.3, 1.7, -0.2)}


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return vr.host(tmp_path_factory.mktemp("volume_host"))


@pytest.fixture(scope="module")
def V(crt):
    return crt.volumes


@pytest.fixture(scope="module")
def built(V, H):
    """name -> the aggregate over the ABI, its image bytes, the restatement, the segments, the phase numbers."""
    out = {}
    for name, regs in vc.aggregates(V).items():
        vol = V.Volumes(regs)
        extent = 4.0 if name == "smoke" else 2.5
        out[name] = dict(vol=vol, image=vol.image_bytes(), ref=vr.VolumesRef(H, vol.records, vol.grid),
                         q=vc.segments(V, N, 11, CENTRES.get(name, (0, 0, 0)), extent), pu=vc.phase_numbers(N, 12))
    return out


NAMES = ["unit_chromatic", "scaled_grey", "rotated_noise", "overlap_homogeneous", "homogeneous_and_grid", "sigma_s_zero",
         "zero_coefficients", "noise_one_octave", "smoke", "nested_eight"]


def test_the_case_list_is_the_one_named(V):
    assert sorted(vc.aggregates(V)) == sorted(NAMES)


# ---- records and image -------------------------------------------------------------------------------------------------
def test_record_sizes_match_the_header(V, tmp_path):
    names = {"CrtVolumeRegion": V.REGION, "CrtVolumeQuery": V.QUERY, "CrtVolumeTransmittance": V.TRANSMITTANCE, "CrtVolumeEvent": V.EVENT}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "crt.h"\nint main(void){' +
                   "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) +
                   'printf("steps %u regions %u\\n", CRT_VOLUME_MAX_STEPS, CRT_VOLUME_MAX_REGIONS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    out = dict(line.split() for line in lines[:4])
    for n, dt in names.items():
        assert int(out[n]) == dt.itemsize, n
    assert (V.REGION.itemsize, V.QUERY.itemsize, V.TRANSMITTANCE.itemsize, V.EVENT.itemsize) == (152, 48, 16, 144)
    assert lines[4] == "steps %d regions %d" % (V.MAX_STEPS, V.MAX_REGIONS) == "steps 65536 regions 8"


def test_the_header_declares_the_six_volume_entry_points(crt):
    """78 declarations before this feature (the documents' running count said 76: it had missed two additions), 84 now."""
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crt.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(crt_[a-z0-9_]+)\s*\(", text))
    assert len(names) == 84 == len(crt.ABI_SYMBOLS)
    for n in ("crt_volumes_new", "crt_volumes_free", "crt_volumes_image", "crt_volumes_density_n", "crt_volumes_transmittance_n",
              "crt_volumes_sample_n"):
        assert n in names and hasattr(crt.lib(), n)


@pytest.mark.parametrize("name", NAMES)
def test_image_is_the_restatements_derived_records(built, V, name):
    b = built[name]
    hd, recs, grid = b["vol"].image()
    assert (hd["magic"], hd["n_regions"], hd["region_bytes"], hd["off_regions"]) == (0x314c4f56, len(b["ref"].regions), 176, 256)
    assert hd["off_grid"] % 256 == 0 and hd["off_grid"] >= 256 + 8 * 176 and hd["bytes"] == len(b["image"]) and hd["grid_floats"] == b["vol"].grid.size
    assert np.array_equal(grid.view(u32), b["vol"].grid.view(u32))
    for reg, rec, src in zip(b["ref"].regions, recs, b["vol"].records):
        for mine, theirs in ((reg.w2l, rec["w2l"]), (reg.half, rec["half"]), (reg.bmin, rec["bmin"]), (reg.bmax, rec["bmax"]),
                             (reg.sigma_s, rec["sigma_s"]), (reg.sigma_a, rec["sigma_a"]), (reg.emission, rec["emission"]),
                             (np.array([reg.majorant, reg.g], f32), np.array([rec["majorant"], rec["g"]], f32))):
            assert np.array_equal(np.asarray(mine, f32).view(u32), np.asarray(theirs, f32).view(u32)), (name, mine, theirs)
        assert rec["field"] == reg.field
        if reg.field == vr.NOISE:
            assert (f32(rec["noise_scale"]), int(rec["noise_octaves"]), f32(rec["noise_gain"]), f32(rec["noise_lacunarity"]),
                    f32(rec["noise_threshold"]), int(rec["noise_seed"])) == reg.noise
        if reg.field == vr.GRID:
            assert (int(rec["nx"]), int(rec["ny"]), int(rec["nz"])) == reg.dims and rec["grid_off"] == src["grid_offset"]


# ---- host twin == restatement, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_density_bits(built, H, name):
    b = built[name]
    rng = np.random.default_rng(5)
    for r, (reg, rec) in enumerate(zip(b["ref"].regions, b["vol"].records)):
        placed = np.array_equal(rec["local_to_world"][:9], np.eye(3, dtype=f32).reshape(-1))
        pts = vc.density_points(rec, 600, 20 + r) if placed else (rng.uniform(-2.5, 2.5, (600, 3)) + rec["local_to_world"][9:12]).astype(f32)
        with np.errstate(all="ignore"):
            want = reg.density(vr.vec(pts))
        got = H.density(b["image"], r, pts)
        assert vr.same_bits(got, want), (name, r, pts[np.nonzero(got.view(u32) != want.view(u32))[0][:3]])
        assert (got[np.isfinite(pts).all(axis=1)] >= 0).all()


def test_density_edge_points_behave_as_the_reference_says(V, H):
    """Exactly on +-half is inside, one ulp outside is 0; a grid holds its edge value within half a voxel of the box;
    points far outside, infinite or not, are 0."""
    img = V.Volumes([V.region(field="grid", grid_dims=(2, 2, 2), grid_data=list(range(8)))]).image_bytes()
    half, out = f32(0.5), np.nextafter(f32(0.5), f32(np.inf))
    pts = np.array([[half, 0, 0], [out, 0, 0], [-half, -half, -half], [0, -out, 0], [-0.45, -0.45, -0.45], [0.45, 0.45, 0.45],
                    [0.3, -0.3, 0.2]], f32)
    got = H.density(img, 0, pts)
    assert got[0] == 3.5 + 0.5 and got[1] == 0 and got[2] == 0.0 and got[3] == 0  # x = +half: the mean of the x1 voxels 1 3 5 7
    assert got[4] == 0.0 and abs(got[5] - 7.0) < 1e-5  # within half a voxel of three edges: the corner voxel's value, not extrapolated
    assert 0 < got[6] < 7
    far = H.density(img, 0, np.array([[1e30, 0, 0], [-1e30, 1e30, 0], [np.inf, 0, 0]], f32))
    assert (far == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_intersect_and_active_intervals_bits(built, H, name):
    b = built[name]
    q = b["q"]
    rays = np.concatenate([q["origin"], q["direction"]], axis=1).astype(f32)
    with np.errstate(all="ignore"):
        for r, reg in enumerate(b["ref"].regions):
            some, t0, t1 = reg.intersect(vr.vec(q["origin"]), vr.vec(q["direction"]))
            g_some, g_t0, g_t1 = H.intersect(b["image"], r, rays)
            assert np.array_equal(some, g_some), (name, r)
            assert vr.same_bits(g_t0[some], t0[some]) and vr.same_bits(g_t1[some], t1[some]), (name, r)
    on, A, B, majorant = b["ref"].active_intervals(q)
    g_on, g_maj, g_A, g_B = H.intervals(b["image"], q)
    R = len(b["ref"].regions)
    assert np.array_equal(g_on[:, :R], on) and not g_on[:, R:].any()
    assert vr.same_bits(g_A[:, :R], A) and vr.same_bits(g_B[:, :R], B) and vr.same_bits(g_maj, majorant)
    if name != "zero_coefficients":
        assert on.any(axis=1).sum() > N // 4 and (~on.any(axis=1)).sum() > N // 20  # segments that cross and segments that miss
    else:
        assert not on[:, 0].any()  # the region without coefficients is skipped


@pytest.mark.parametrize("name", NAMES)
def test_transmittance_bits(built, H, V, name):
    b = built[name]
    want = b["ref"].transmittance(b["q"], V.TRANSMITTANCE)
    got = H.transmittance(b["image"], b["q"], V.TRANSMITTANCE)
    bad = vr.record_mismatches(got, want, ["transmittance", "status"])
    assert len(bad) == 0, (name, len(bad), b["q"][bad[:2]], got[bad[:2]], want[bad[:2]])
    assert (got["status"] == 0).all()
    assert (got["transmittance"] == 1).all(axis=1).any()
    assert (got["transmittance"] < 1).any() or name == "noise_one_octave"  # threshold 0.999 carves the whole field away


@pytest.mark.parametrize("name", NAMES)
def test_sample_interaction_and_phase_mixture_bits(built, H, V, name):
    b = built[name]
    want = b["ref"].sample(b["q"], b["pu"], V.EVENT)
    got = H.sample(b["image"], b["q"], b["pu"], V.EVENT)
    bad = vr.record_mismatches(got, want, EVENT_FIELDS)
    assert len(bad) == 0, (name, len(bad), b["q"][bad[:2]], got[bad[:2]], want[bad[:2]])
    assert (got["status"] == 0).all()
    sc = got["kind"] == V.SCATTER
    if name in ("overlap_homogeneous", "sigma_s_zero", "noise_one_octave"):  # sigma_s = 0 (or a field that is 0): p_scatter = 0
        assert not sc.any()
    else:
        assert sc.sum() > 100 and (got["n_lobes"][sc] >= 1).all() and (got["pdf"][sc] >= f32(1e-6)).all()
        assert np.allclose(got["lobes"][sc][:, :, 0].sum(axis=1), 1.0, atol=1e-5)
        assert np.allclose(np.linalg.norm(got["dir"][sc], axis=1), 1.0, atol=1e-5)
    # without phase numbers: the same events, no direction
    bare = H.sample(b["image"], b["q"], None, V.EVENT)
    assert len(vr.record_mismatches(bare, got, [f for f in EVENT_FIELDS if f not in ("dir", "pdf")])) == 0
    assert not bare["dir"].any() and not bare["pdf"].any()


def test_special_weights_and_lobes(built, H, V):
    """sigma_a = 0 and grey: a scatter's weight is exactly 1; chromatic coefficients: the channels differ; eight nested
    scattering regions: the lobe array fills; emission off: nothing is emitted."""
    g = H.sample(built["scaled_grey"]["image"], built["scaled_grey"]["q"], None, V.EVENT)
    assert (g["weight"][g["kind"] == 1] == 1.0).all() and not g["emitted"].any()
    c = H.sample(built["unit_chromatic"]["image"], built["unit_chromatic"]["q"], None, V.EVENT)
    sc = c["kind"] == 1
    assert (c["weight"][sc][:, 0] != c["weight"][sc][:, 2]).any() and (c["emitted"][sc] > 0).any()
    n8 = H.sample(built["nested_eight"]["image"], built["nested_eight"]["q"], None, V.EVENT)
    assert n8["n_lobes"].max() == 8
    z = H.sample(built["sigma_s_zero"]["image"], built["sigma_s_zero"]["q"], None, V.EVENT)
    assert (z["emitted"] > 0).any() and (z["kind"] == 0).all()


def test_hg_phase_bits(H):
    c, g = np.meshgrid(np.linspace(-1, 1, 401, dtype=f32), np.array([-0.99, -0.4, -1e-4, 0.0, 0.2, 0.4, 0.99], f32))
    with np.errstate(all="ignore"):
        assert vr.same_bits(H.hg_phase(c, g), vr.hg_phase(H, c.reshape(-1), g.reshape(-1)))


def test_largest_candidate_count_is_far_below_the_limit(built, V):
    """The limit cannot be what makes a parity case pass: the restatement counts every walk's collision candidates."""
    worst = 0
    for name in NAMES:
        b = built[name]
        b["ref"].transmittance(b["q"], V.TRANSMITTANCE)
        b["ref"].sample(b["q"], None, V.EVENT)
        print("%s: largest candidate count %d" % (name, b["ref"].max_candidates))
        worst = max(worst, b["ref"].max_candidates)
    assert 0 < worst < V.MAX_STEPS // 16, worst


# ---- the step limit (host twin only) -------------------------------------------------------------------------------------
def test_step_limit_on_walks_that_never_end(H, V):
    """A NaN origin (no box clips the segment) and a zero direction (the local direction is below 1e-9 on every axis),
    both with t_max = inf over a region of null collisions only: the reference's loops never end; here both walks come
    back CRT_VOLUME_STEP_LIMIT with zeros. And the walk that ends by itself after about 4 * MAX_STEPS candidates."""
    regions, q1 = vc.step_limit_aggregate(V)
    vol = V.Volumes(regions)
    q = np.zeros(3, V.QUERY)
    q[0] = q1[0]
    q["origin"][1], q["direction"][1] = np.nan, (1, 0, 0)
    q["origin"][2], q["direction"][2] = (0, 0, -0.3), (0, 0, 0)
    q["t_eps"], q["seed"] = 1e-3, (1, 2, 3)
    q["t_max"][1:] = np.inf
    t = H.transmittance(vol.image_bytes(), q, V.TRANSMITTANCE)
    e = H.sample(vol.image_bytes(), q, vc.phase_numbers(3, 1), V.EVENT)
    assert (t["status"] == V.STEP_LIMIT).all() and not t["transmittance"].any()
    assert (e["status"] == V.STEP_LIMIT).all() and (e["kind"] == V.PASSTHROUGH).all()
    for f in ("p", "t", "weight", "emitted", "n_lobes", "dir", "pdf", "lobes"):
        assert not e[f].any(), f


# ---- the reference's unit tests (volume.rs:561-799) on the host twin ---------------------------------------------------
def _x_ray(V, n=1, t_max=10.0):
    q = np.zeros(n, V.QUERY)
    q["origin"], q["direction"], q["t_eps"], q["t_max"] = (-2, 0, 0), (1, 0, 0), 1e-3, t_max
    q["seed"] = (np.arange(n, dtype=np.uint64) * 2654435761 + 0xC0FFEE).astype(u32)
    return q


def test_ref_homogeneous_transmittance_is_exact_beer_lambert(H, V):
    vol = V.Volumes([V.region(sigma_s=0.7, sigma_a=(0.2, 0.4, 0.9))])
    q = _x_ray(V, 2)
    tr = H.transmittance(vol.image_bytes(), q, V.TRANSMITTANCE)["transmittance"]
    expect = np.exp(-(np.float64(0.7) + np.array([0.2, 0.4, 0.9])))
    assert np.abs(tr[0] - expect).max() < 1e-5
    assert np.array_equal(tr[0], tr[1])  # the fast path is deterministic: another seed, the same value


def test_ref_ratio_tracking_matches_analytic_on_grid(H, V):
    d = 0.6
    vol = V.Volumes([V.region(sigma_s=(0.3, 0.5, 0.8), sigma_a=0.4, field="grid", grid_dims=(4, 4, 4), grid_data=[d] * 64)])
    tr = H.transmittance(vol.image_bytes(), _x_ray(V, 20000), V.TRANSMITTANCE)
    assert (tr["status"] == 0).all()
    mean = tr["transmittance"].astype(np.float64).mean(axis=0)
    expect = np.exp(-(np.array([0.3, 0.5, 0.8]) + 0.4) * d)
    assert np.abs(mean - expect).max() < 0.01, (mean, expect)


def test_ref_delta_tracking_scatter_probability_matches_analytic(H, V):
    sigma = 1.3
    vol = V.Volumes([V.region(sigma_s=sigma, sigma_a=0.0)])
    e = H.sample(vol.image_bytes(), _x_ray(V, 20000), None, V.EVENT)
    sc = e["kind"] == V.SCATTER
    assert np.abs(e["weight"][sc] - 1.0).max() < 1e-5
    observed, expect = sc.mean(), 1.0 - np.exp(-sigma)
    assert abs(observed - expect) < 0.01, (observed, expect)


def test_ref_emission_walk_matches_analytic_slab(H, V):
    sigma_a, le = 0.8, np.array([4.0, 1.5, 0.3])
    vol = V.Volumes([V.region(sigma_s=0.0, sigma_a=sigma_a, emission=le)])
    e = H.sample(vol.image_bytes(), _x_ray(V, 40000), None, V.EVENT)
    mean = e["emitted"].astype(np.float64).mean(axis=0)
    expect = le * (1.0 - np.exp(-sigma_a))
    assert np.abs((mean - expect) / expect).max() < 0.03, (mean, expect)


def test_ref_grid_trilinear_exact_at_centers(H, V):
    data = [float(i) for i in range(8)]
    vol = V.Volumes([V.region(field="grid", grid_dims=(2, 2, 2), grid_data=data)])
    img = vol.image_bytes()
    for z in range(2):
        for y in range(2):
            for x in range(2):
                u = np.array([[0.25 + 0.5 * x, 0.25 + 0.5 * y, 0.25 + 0.5 * z]], f32)
                assert abs(H.density(img, 0, u - f32(0.5))[0] - data[x + 2 * (y + 2 * z)]) < 1e-6
    assert abs(H.density(img, 0, np.zeros((1, 3), f32))[0] - 3.5) < 1e-6  # the box centre: the mean of all 8 samples


def test_ref_noise_deterministic_and_bounded_by_majorant(H, V):
    vol = V.Volumes([V.region(field="noise", noise_scale=4.0, noise_octaves=4, noise_gain=0.5, noise_lacunarity=2.0,
                              noise_threshold=0.3, noise_seed=42)])
    img = vol.image_bytes()
    i = np.arange(1000, dtype=u32)
    one = lambda k: np.full(1000, k, u32)
    seven = np.array([7], u32)
    u = np.stack([vr.hash3(i, one(1), one(2), seven), vr.hash3(i, one(3), one(4), seven), vr.hash3(i, one(5), one(6), seven)], axis=1)
    first, second = H.density(img, 0, u - f32(0.5)), H.density(img, 0, u - f32(0.5))
    assert ((first >= 0) & (first <= 1.0)).all()  # max_value() of a noise field is 1
    assert np.array_equal(first, second) and (first > 0).any()


def test_ref_oriented_box_interval_in_world_units(H, V):
    ray = np.array([[-2, 0, 0, 1, 0, 0]], f32)
    scaled = V.Volumes([V.region(local_to_world=vc.affine((2, 1, 1), 0, (5, 0, 0)), half_extent=1.0, sigma_s=1.0)])
    some, t0, t1 = H.intersect(scaled.image_bytes(), 0, ray)
    assert some[0] and abs(t0[0] - 5.0) < 1e-4 and abs(t1[0] - 9.0) < 1e-4
    rotated = V.Volumes([V.region(local_to_world=vc.affine((1, 1, 1), 45, (0, 0, 0)), half_extent=1.0, sigma_s=1.0)])
    some, t0, t1 = H.intersect(rotated.image_bytes(), 0, ray)
    s = np.sqrt(f32(2.0))
    assert some[0] and abs(t0[0] - (2.0 - s)) < 1e-4 and abs(t1[0] - (2.0 + s)) < 1e-4


def test_ref_overlapping_regions_compose_exactly(H, V):
    vol = V.Volumes([V.region(sigma_s=0.0, sigma_a=0.5), V.region(local_to_world=vc.affine(translate=(0.25, 0, 0)), sigma_s=0.0, sigma_a=0.75)])
    tr = H.transmittance(vol.image_bytes(), _x_ray(V), V.TRANSMITTANCE)["transmittance"]
    assert abs(tr[0, 0] - np.exp(-0.5 - 0.75)) < 1e-5


def test_ref_phase_mix_pdf_matches_single_lobe(H, V):
    """PhaseMix::single(0.4).pdf(mu) == hg_phase(mu, 0.4): the mixture of a one-region scatter, at the cosines the
    reference lists (through hg_phase itself) and at the sampled directions (through the scatter record)."""
    vol = V.Volumes([V.region(sigma_s=3.0, sigma_a=0.0, g=0.4)])
    q = _x_ray(V, 500)
    pu = vc.phase_numbers(500, 3)
    e = H.sample(vol.image_bytes(), q, pu, V.EVENT)
    sc = e["kind"] == V.SCATTER
    assert sc.sum() > 300 and (e["n_lobes"][sc] == 1).all() and (e["lobes"][sc][:, 0, 0] == 1.0).all() and (e["lobes"][sc][:, 0, 1] == f32(0.4)).all()
    mu = e["dir"][sc][:, 0]  # wi = +x
    assert np.abs(e["pdf"][sc] - H.hg_phase(mu, np.full(mu.size, 0.4, f32))).max() < 1e-7
    for m in (-0.9, -0.2, 0.0, 0.5, 0.99):
        want = (1 - 0.16) / (4 * np.pi * (1 + 0.16 - 0.8 * m) ** 1.5)
        assert abs(H.hg_phase([m], [0.4])[0] - want) < 1e-6 * max(want, 1)


# ---- USD import (usd_scene.rs:192-271) -----------------------------------------------------------------------------------
def _load(crt, name, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        desc = crt.usda.load(os.path.join(GOLDEN, name), **kw)
    return desc, [str(x.message) for x in w]


def test_loads_fog_usda(crt, H, V):
    desc, warned = _load(crt, "fog.usda", volumes=True)
    assert (len(desc.geoms), len(desc.lights), len(desc.volumes)) == (3, 1, 1) and not warned
    fog = desc.volumes[0]
    assert fog["field"] == "homogeneous" and abs(fog["g"] - 0.3) < 1e-6 and np.abs(np.array(fog["sigma_s"]) - 0.15).max() < 1e-6
    vol = crt.usda.build_volumes(desc, crt)
    _, recs, _ = vol.image()
    assert recs[0]["field"] == V.HOMOGENEOUS and abs(recs[0]["g"] - 0.3) < 1e-6 and np.abs(recs[0]["sigma_s"] - 0.15).max() < 1e-6
    q = np.zeros(1, V.QUERY)
    q["origin"], q["direction"], q["t_eps"], q["t_max"], q["seed"] = (0, 2, 10), (0, 0, -1), 1e-3, 100.0, 1
    tr = H.transmittance(vol.image_bytes(), q, V.TRANSMITTANCE)["transmittance"]
    assert abs(tr[0, 0] - np.exp(-(0.15 + 0.01) * 4.0)) < 1e-4


def test_loads_smoke_usda(crt, H, V):
    desc, warned = _load(crt, "smoke.usda", volumes=True)
    assert (len(desc.geoms), len(desc.lights), len(desc.volumes)) == (2, 1, 3) and not warned
    vol = crt.usda.build_volumes(desc, crt)
    _, recs, _ = vol.image()
    smoke = [r for r in recs if r["field"] != V.HOMOGENEOUS and abs(r["g"] - 0.2) < 1e-6]
    assert len(smoke) == 1 and abs(smoke[0]["sigma_s"][0] - 9.6) < 1e-4  # densityScale folded in: 0.8 * 12
    ember = [r for r in recs if r["emission"].max() > 0]
    assert len(ember) == 1 and ember[0]["field"] == V.HOMOGENEOUS
    grid = [k for k, r in enumerate(recs) if r["field"] != V.HOMOGENEOUS and abs(r["g"]) < 1e-6]
    assert len(grid) == 1
    centre = np.array([1.1, 2.6, -0.8], f32)
    d = H.density(vol.image_bytes(), grid[0], np.stack([centre, centre + f32(0.49)]))
    assert d[0] > 0.3 and d[1] < 1e-3
    # the importer's records are the hand-built smoke aggregate of the case list
    want = V.Volumes(vc.aggregates(V)["smoke"])
    order = [n for n in ("Smoke", "Ember", "GridPuff")]
    got = {r["name"]: k for k, r in enumerate(desc.volumes)}
    assert sorted(got) == sorted(order)
    for k, n in enumerate(order):
        a, b = vol.records[got[n]].copy(), want.records[k].copy()
        a["grid_offset"] = b["grid_offset"] = 0
        assert a.tobytes() == b.tobytes(), n


def test_importer_default_sees_no_volume_and_the_geometry_it_saw(crt):
    for name in ("fog.usda", "smoke.usda"):
        plain, warned = _load(crt, name)
        asked, _ = _load(crt, name, volumes=True)
        assert plain.volumes == [] and not warned  # ignored as before, without a new warning
        assert [g["name"] for g in plain.geoms] == [g["name"] for g in asked.geoms]  # a Cube was never geometry
        for a, b in zip(plain.geoms, asked.geoms):
            assert a["kind"] == b["kind"] and all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))
        assert len(plain.lights) == len(asked.lights) == 1


SKIP_STAGE = """#usda 1.0
def Xform "World"
{
    def Camera "Cam"
    {
        float focalLength = 24
    }
    def Cube "Unknown" { token crust:volume:type = "plasma" }
    def Cube "NoData" { token crust:volume:type = "grid"
        int[] crust:volume:gridDims = [2, 2, 2] }
    def Cube "TwoDims" { token crust:volume:type = "grid"
        int[] crust:volume:gridDims = [2, 2]
        float[] crust:volume:gridData = [1, 2, 3, 4] }
    def Cube "Mismatch" { token crust:volume:type = "grid"
        int[] crust:volume:gridDims = [2, 2, 2]
        float[] crust:volume:gridData = [1, 2, 3] }
    def Mesh "FogMesh"
    {
        token crust:volume:type = "homogeneous"
        int[] faceVertexCounts = [3]
        int[] faceVertexIndices = [0, 1, 2]
        point3f[] points = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    }
    def Cube "Defaults" { token crust:volume:type = "smoke" }
    def PointInstancer "Inst"
    {
        int[] protoIndices = [0]
        point3f[] positions = [(0, 0, 0)]
        rel prototypes = [</World/Inst/Proto>]
        def Xform "Proto"
        {
            def Sphere "Ball" { double radius = 1 }
            def Cube "Inner" { token crust:volume:type = "homogeneous" }
        }
    }
}
"""


def test_importer_skip_cases_warn(crt, tmp_path):
    path = tmp_path / "skips.usda"
    path.write_text(SKIP_STAGE)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        desc = crt.usda.load(str(path), volumes=True)
    text = [str(x.message) for x in w]
    for needle in ("unknown crust:volume:type", "NoData: grid type needs", "TwoDims: grid type needs", "does not match gridData length 3",
                   "Inner is inside a prototype"):
        assert sum(needle in t for t in text) == 1, (needle, text)
    assert [v["name"] for v in desc.volumes] == ["Defaults", "FogMesh"] or [v["name"] for v in desc.volumes] == ["FogMesh", "Defaults"]
    assert "FogMesh" not in [g.get("name") for g in desc.geoms]  # a volume prim is never geometry
    d = [v for v in desc.volumes if v["name"] == "Defaults"][0]
    assert (d["sigma_s"], d["sigma_a"], d["g"], d["density_scale"], d["half_extent"]) == ((0.5,) * 3, (0.0,) * 3, 0.0, 1.0, (0.5,) * 3)
    assert (d["noise_scale"], d["noise_octaves"], d["noise_gain"], d["noise_lacunarity"], d["noise_threshold"], d["noise_seed"]) == (4.0, 4, 0.5, 2.0, 0.3, 0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        plain = crt.usda.load(str(path))
    assert plain.volumes == [] and not [x for x in w if "olume" in str(x.message)]
    assert "FogMesh" in [g.get("name") for g in plain.geoms]  # read by its schema, as before


# ---- refusals and argument checks ----------------------------------------------------------------------------------------
def test_every_refusal_returns_null_with_its_reason(crt, V):
    L = crt.lib()

    def refused(regions, needle, grid=None, grid_len=None):
        recs, g = V.pack_regions(regions) if not isinstance(regions, tuple) else regions
        if grid is not None:
            g = np.asarray(grid, f32)
        n = g.size if grid_len is None else grid_len
        h = L.crt_volumes_new(C.c_void_p(recs.ctypes.data), len(recs), crt._fp(g) if g.size else None, n)
        assert not h, needle
        assert needle in L.crt_last_error().decode(), (needle, L.crt_last_error())
        if grid_len is None:
            with pytest.raises(crt.CrtError, match="crt_volumes_new"):
                V.Volumes((recs, g))

    refused([V.region()] * 9, "9 regions")
    for key in ("sigma_s", "sigma_a", "emission", "half_extent", "g", "density_scale", "noise_scale", "noise_gain",
                "noise_lacunarity", "noise_threshold"):
        refused([V.region(**{key: np.nan})], "not finite")
    m = vc.affine()
    m[10] = np.inf
    refused([V.region(local_to_world=m)], "not finite")
    refused([V.region(field=5)], "unknown field kind 5")
    refused([V.region(field="noise", noise_octaves=33)], "33 noise octaves")
    refused([V.region(field="grid", grid_dims=(2, 2, 3), grid_data=range(8))], "2 x 2 x 3 grid over 8 values")
    refused([V.region(field="grid", grid_dims=(2, 0, 2), grid_data=[])], "2 x 0 x 2 grid over 0 values")
    refused([V.region(field="grid", grid_dims=(0xffffffff,) * 3, grid_data=range(8))], "grid over 8 values")
    recs, g = V.pack_regions([V.region(field="grid", grid_dims=(2, 2, 2), grid_data=range(8))])
    recs["grid_offset"] = 1
    refused((recs, g), "reads grid values 1 .. 9 of 8")
    recs["grid_offset"] = 0
    refused((recs, g), "without an array", grid=np.zeros(0, f32), grid_len=8)
    singular = vc.affine((0, 1, 1))
    refused([V.region(local_to_world=singular)], "no finite inverse")
    # a region whose majorant is <= 0 is accepted (and skipped by the walk), as is an empty aggregate
    assert V.Volumes([V.region(sigma_s=0.0, sigma_a=0.0)]).image()[1]["majorant"][0] == 0
    assert V.Volumes([]).image()[0]["n_regions"] == 0
    # ... and refusing leaks nothing: handles come and go
    for _ in range(200):
        V.Volumes([V.region()]).close()


def test_argument_checks_of_the_batched_forms_need_no_device(crt, V):
    L = crt.lib()
    vol = V.Volumes([V.region()])
    assert L.crt_volumes_transmittance_n(vol.h, None, 0, None, None) == 0 and L.crt_volumes_sample_n(vol.h, None, None, 0, None, None) == 0
    assert L.crt_volumes_density_n(vol.h, 0, None, 0, None, None) == 0          # n == 0
    assert L.crt_volumes_transmittance_n(vol.h, None, 5, None, None) == -1 and L.crt_volumes_sample_n(vol.h, None, None, 5, None, None) == -1
    assert L.crt_volumes_density_n(vol.h, 0, None, 5, None, None) == -1         # queries / results missing
    assert L.crt_volumes_density_n(vol.h, 1, 1, 5, 1, None) == -1 and b"region 1 of 1" in L.crt_last_error()
    assert L.crt_volumes_transmittance_n(None, 1, 5, 1, None) == -1 and L.crt_volumes_sample_n(None, 1, None, 5, 1, None) == -1
    assert L.crt_volumes_density_n(None, 0, 1, 5, 1, None) == -1 and L.crt_volumes_image(None, None, None) == -1
    L.crt_volumes_free(None)  # as free(NULL)


# ---- sanitizers: a stand-alone program, on the CPU ---------------------------------------------------------------------
def test_builder_refusals_and_bounded_walks_are_clean_under_asan_and_ubsan(tmp_path):
    """profiles/host_shade/volume_sanitize.cpp: volumes.cpp's builder and the host-compiled walks in a program of their
    own (its own main), built with -fsanitize=address,undefined; nothing of it is loaded into Python."""
    exe = tmp_path / "volume_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "profiles", "host_shade"),
           "-I" + os.path.join(ROOT, "crust-render_amd", "csrc"), os.path.join(ROOT, "profiles", "host_shade", "volume_sanitize.cpp"),
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "volume_sanitize: 13 refusals, 4 bounded walks, 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
