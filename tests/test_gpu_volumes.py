"""Volume regions on the GPU: crt_volumes_density_n / _transmittance_n / _sample_n against the float32 restatement of
volume.rs (tests/volume_ref.py) bit for bit — status, kind, lobes and phase outputs included — the two USD samples'
aggregates through the seam, the reference's three statistical unit tests once more through the device, determinism
across streams, and the step limit on the one walk that ends by itself. The CPU half is tests/test_volumes.py."""
import os

import numpy as np
import pytest

import volume_cases as vc
import volume_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
f32, u32 = np.float32, np.uint32
SIZES = [1, 63, 64, 65, 257, 20003]  # below, at and above a wave; more than one block; many blocks with a ragged last one
BIG = 20003
EVENT_FIELDS = ["p", "t", "weight", "kind", "emitted", "n_lobes", "dir", "pdf", "lobes", "status"]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return vr.host(tmp_path_factory.mktemp("volume_host"))


@pytest.fixture(scope="module")
def V(crt):
    return crt.volumes


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _smoke_from_usd(crt):
    desc = crt.usda.load(os.path.join(GOLDEN, "smoke.usda"), volumes=True)
    return crt.usda.build_volumes(desc, crt)


@pytest.fixture(scope="module")
def big(crt, V, H):
    """The two 20 003-segment workloads, their restatement computed once: eight nested regions of every field kind, and
    smoke.usda's three regions as the importer builds them."""
    out = {}
    for name, vol, centre, extent in (("nested_eight", V.Volumes(vc.aggregates(V)["nested_eight"]), (0, 0, 0), 2.5),
                                      ("smoke_usd", _smoke_from_usd(crt), (0.3, 1.7, -0.2), 4.0)):
        ref = vr.VolumesRef(H, vol.records, vol.grid)
        q, pu = vc.segments(V, BIG, 31, centre, extent), vc.phase_numbers(BIG, 32)
        out[name] = dict(vol=vol, ref=ref, q=q, pu=pu, want_t=ref.transmittance(q, V.TRANSMITTANCE), want_s=ref.sample(q, pu, V.EVENT))
    return out


def _compare(V, vol, q, pu, want_t, want_s):
    import torch
    d_q = V.to_device(q)
    got_t = _host(vol.transmittance(d_q), V.TRANSMITTANCE)
    got_s = _host(vol.sample(d_q, torch.from_numpy(pu).cuda()), V.EVENT)
    torch.cuda.synchronize()
    bad = vr.record_mismatches(got_t, want_t, ["transmittance", "status"])
    assert len(bad) == 0, (len(bad), q[bad[:2]], got_t[bad[:2]], want_t[bad[:2]])
    bad = vr.record_mismatches(got_s, want_s, EVENT_FIELDS)
    assert len(bad) == 0, (len(bad), q[bad[:2]], got_s[bad[:2]], want_s[bad[:2]])
    assert not got_s["_pad"].any()
    return got_t, got_s


@pytest.mark.parametrize("n", SIZES)
def test_seam_equals_the_restatement_at_every_launch_size(V, big, n):
    import torch
    b = big["nested_eight"]
    got_t, got_s = _compare(V, b["vol"], b["q"][:n], b["pu"][:n], b["want_t"][:n], b["want_s"][:n])
    if n == BIG:
        sc = got_s["kind"] == V.SCATTER
        assert sc.sum() > BIG // 4 and (~sc).sum() > BIG // 10 and got_s["n_lobes"].max() == 8 and (got_s["status"] == 0).all()
        assert (got_t["transmittance"] < 1).any() and (got_t["transmittance"] == 1).all(axis=1).any()
    # density of every region at n points around it
    for r, (reg, rec) in enumerate(zip(b["ref"].regions, b["vol"].records)):
        pts = (np.random.default_rng(100 + r).uniform(-1.5, 1.5, (n, 3)) * (rec["half_extent"] * 1.3)).astype(f32)
        pts[:min(n, 3)] = np.array([[np.nan, 0, 0], [1e30, -1e30, 0], [0, 0, 0]], f32)[:min(n, 3)]
        with np.errstate(all="ignore"):
            want = reg.density(vr.vec(pts))
        got = b["vol"].density(r, torch.from_numpy(pts).cuda()).cpu().numpy()
        assert vr.same_bits(got, want), (r, n)


@pytest.mark.parametrize("name", ["unit_chromatic", "scaled_grey", "rotated_noise", "overlap_homogeneous", "homogeneous_and_grid",
                                  "sigma_s_zero", "zero_coefficients", "noise_one_octave", "smoke"])
def test_every_aggregate_of_the_case_list(V, H, name):
    """The remaining aggregates at 2 000 segments (eight blocks, the last one ragged), density edge points included."""
    import torch
    vol = V.Volumes(vc.aggregates(V)[name])
    ref = vr.VolumesRef(H, vol.records, vol.grid)
    centre = {"scaled_grey": (5, 0, 0), "smoke": (0.3, 1.7, -0.2)}.get(name, (0, 0, 0))
    q, pu = vc.segments(V, 2000, 11, centre, 4.0 if name == "smoke" else 2.5), vc.phase_numbers(2000, 12)
    _compare(V, vol, q, pu, ref.transmittance(q, V.TRANSMITTANCE), ref.sample(q, pu, V.EVENT))
    for r, (reg, rec) in enumerate(zip(ref.regions, vol.records)):
        if np.array_equal(rec["local_to_world"][:9], np.eye(3, dtype=f32).reshape(-1)):
            pts = vc.density_points(rec, 300, 20 + r)
            with np.errstate(all="ignore"):
                want = reg.density(vr.vec(pts))
            assert vr.same_bits(vol.density(r, torch.from_numpy(pts).cuda()).cpu().numpy(), want), (name, r)


def test_usd_samples_through_the_seam(crt, V, big):
    """fog.usda: exact Beer-Lambert through the 4-unit room (usd_scene.rs:192-228); smoke.usda: 20 003 seeded segments
    through its three regions == the restatement."""
    desc = crt.usda.load(os.path.join(GOLDEN, "fog.usda"), volumes=True)
    fog = crt.usda.build_volumes(desc, crt)
    q = np.zeros(1, V.QUERY)
    q["origin"], q["direction"], q["t_eps"], q["t_max"], q["seed"] = (0, 2, 10), (0, 0, -1), 1e-3, 100.0, 1
    tr = _host(fog.transmittance(V.to_device(q)), V.TRANSMITTANCE)
    assert tr["status"][0] == 0 and abs(tr["transmittance"][0, 0] - np.exp(-(0.15 + 0.01) * 4.0)) < 1e-4
    b = big["smoke_usd"]
    got_t, got_s = _compare(V, b["vol"], b["q"], b["pu"], b["want_t"], b["want_s"])
    assert (got_s["kind"] == V.SCATTER).sum() > 1000 and (got_s["emitted"] > 0).any() and len(b["vol"].records) == 3


def _x_ray(V, n):
    q = np.zeros(n, V.QUERY)
    q["origin"], q["direction"], q["t_eps"], q["t_max"] = (-2, 0, 0), (1, 0, 0), 1e-3, 10.0
    q["seed"] = (np.arange(n, dtype=np.uint64) * 2654435761 + 0xC0FFEE).astype(u32)
    return q


def test_the_reference_statistical_unit_tests_through_the_device(V):
    """volume.rs:583-673 with their counts and tolerances: ratio tracking on a constant grid (20 000 walks, 0.01), the
    scatter probability 1 - e^-1.3 (20 000, 0.01; weight 1 within 1e-5), the emissive slab (40 000, 3 % relative)."""
    d = 0.6
    grid = V.Volumes([V.region(sigma_s=(0.3, 0.5, 0.8), sigma_a=0.4, field="grid", grid_dims=(4, 4, 4), grid_data=[d] * 64)])
    tr = _host(grid.transmittance(V.to_device(_x_ray(V, 20000))), V.TRANSMITTANCE)
    mean, expect = tr["transmittance"].astype(np.float64).mean(axis=0), np.exp(-(np.array([0.3, 0.5, 0.8]) + 0.4) * d)
    assert (tr["status"] == 0).all() and np.abs(mean - expect).max() < 0.01, (mean, expect)
    sigma = 1.3
    e = _host(V.Volumes([V.region(sigma_s=sigma, sigma_a=0.0)]).sample(V.to_device(_x_ray(V, 20000))), V.EVENT)
    sc = e["kind"] == V.SCATTER
    assert np.abs(e["weight"][sc] - 1.0).max() < 1e-5 and abs(sc.mean() - (1.0 - np.exp(-sigma))) < 0.01, sc.mean()
    sigma_a, le = 0.8, np.array([4.0, 1.5, 0.3])
    e = _host(V.Volumes([V.region(sigma_s=0.0, sigma_a=sigma_a, emission=le)]).sample(V.to_device(_x_ray(V, 40000))), V.EVENT)
    mean, expect = e["emitted"].astype(np.float64).mean(axis=0), le * (1.0 - np.exp(-sigma_a))
    assert np.abs((mean - expect) / expect).max() < 0.03, (mean, expect)


def test_two_launches_on_two_streams_give_identical_bytes(V, big):
    import torch
    b = big["nested_eight"]
    d_q, d_pu = V.to_device(b["q"]), torch.from_numpy(b["pu"]).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a_s, a_t = b["vol"].sample(d_q, d_pu, stream=s1), b["vol"].transmittance(d_q, stream=s1)
    with torch.cuda.stream(s2):
        b_s, b_t = b["vol"].sample(d_q, d_pu, stream=s2), b["vol"].transmittance(d_q, stream=s2)
    torch.cuda.synchronize()
    assert torch.equal(a_s, b_s) and torch.equal(a_t, b_t) and a_s.numel() == BIG * V.EVENT.itemsize


def test_step_limit_on_the_walk_that_ends_by_itself(V, H):
    """A pure-null-collision region whose majorant optical depth over the segment is 4 * MAX_STEPS (tests/volume_cases.py,
    step_limit_aggregate): the reference's walk would finish after about 262 000 candidates; the bounded walk stops at
    65 536 with CRT_VOLUME_STEP_LIMIT and zeros. A broken bound shows as a wrong status, never as a hang."""
    regions, q = vc.step_limit_aggregate(V)
    vol = V.Volumes(regions)
    assert vol.image()[1]["majorant"][0] == 4.0 * V.MAX_STEPS
    t = _host(vol.transmittance(V.to_device(q)), V.TRANSMITTANCE)
    e = _host(vol.sample(V.to_device(q)), V.EVENT)
    assert t["status"][0] == V.STEP_LIMIT and not t["transmittance"].any()
    assert e["status"][0] == V.STEP_LIMIT and e["kind"][0] == V.PASSTHROUGH
    for f in ("p", "t", "weight", "emitted", "n_lobes", "dir", "pdf", "lobes"):
        assert not e[f].any(), f
    assert t.tobytes() == H.transmittance(vol.image_bytes(), q, V.TRANSMITTANCE).tobytes()
    assert e.tobytes() == H.sample(vol.image_bytes(), q, None, V.EVENT).tobytes()
