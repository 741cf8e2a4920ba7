"""Volume renders without a device: the volume-aware forward integrator (tests/volume_pt/volume_pt.c) that the wavefront
renderer's volume renders are compared with (tests/test_gpu_volume_render.py) is pinned here —
  1. to the oracle where the oracle is the truth: no region crossed, per-sample radiance bits and all eight RayStats;
  2. to independent walks: the same image with every aggregate call answered by the numpy restatement volume_ref.VolumesRef;
  3. to physics: Beer-Lambert through an absorbing slab, and the white furnace under each of the four strategies —
and the launch plan with volumes (launch_plan.h, plan_launches) is swept on the CPU, the new ABI entry checked."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ora
import ora_world
import volume_pt as vp
import volume_ref as vr
import volume_render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32, f32 = np.uint32, np.float32


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("volume_pt")


@pytest.fixture(scope="module")
def host(work):
    return vr.host(work)


def stats_tuple(st):
    return tuple(int(getattr(st, f)) for f, _t in ora.RayStats._fields_)


# ---- 1. the restatement equals the oracle where the oracle is the truth ------------------------------------------------
@pytest.mark.parametrize("scene,w,h,depth", [("cornellbox", 32, 32, 8), ("veach_mis", 40, 24, 8), ("sun_sky", 40, 24, 8)])
@pytest.mark.parametrize("aggregate", ["empty", "uncrossed"])
def test_restatement_equals_the_oracle_where_no_region_is_crossed(crt, oracle, work, host, scene, w, h, depth, aggregate):
    desc = crt.usda.load(rc.scene_file(scene), w, h)
    o = ora_world.OracleRenderer(desc, crt.usda, max_depth=depth, forward=1)
    vol = crt.volumes.Volumes([] if aggregate == "empty" else rc.far_away(crt.volumes))
    vi = vp.VolumeIntegrator(work, o, vp.host_table(host, vol.image_bytes()))
    st, ost, cov = ora.RayStats(), ora.RayStats(), vp.Coverage()
    rgb = np.zeros(3, f32)
    for j in range(h):
        for i in range(w):
            for s in range(4):
                got = vi.render_sample(i, j, s, st, cov)
                oracle.lib().ora_render_sample(C.byref(o.job), i, j, s, ora._fp(rgb), C.byref(ost))
                assert np.array_equal(got.view(u32), rgb.view(u32)), (scene, aggregate, i, j, s, got, rgb)
    assert stats_tuple(st) == stats_tuple(ost), (scene, aggregate)
    assert not any(cov.as_dict().values()), cov.as_dict()  # no arm of the volume form ran
    # ... and the frame entry point (render_pixel, the workers) gives the oracle's frame
    img, counts, fst, _cov = vi.render(4)
    oimg, ofst = o.render(4, forward=1)
    assert np.array_equal(img.view(u32), oimg.view(u32)) and stats_tuple(fst) == stats_tuple(ofst) and (counts == 4).all()


# ---- 2. independent walks --------------------------------------------------------------------------------------------
def test_independent_walks_give_the_same_image(crt, oracle, work, host):
    """fog, 16 x 12 x 1, depth 4: the function table routed to the numpy restatement of the reference's Volumes instead of
    the host-compiled device source."""
    desc = crt.usda.load(rc.scene_file("fog"), 16, 12, volumes=True)
    o = ora_world.OracleRenderer(desc, crt.usda, max_depth=4)
    vol = crt.usda.build_volumes(desc, crt)
    a = vp.VolumeIntegrator(work, o, vp.host_table(host, vol.image_bytes())).render(1)
    ref = vr.VolumesRef(host, vol.records, vol.grid)
    b = vp.VolumeIntegrator(work, o, vp.ref_table(ref, host, crt.volumes)).render(1, threads=1)
    assert a[3]["phase_vertices"] > 0 and a[3]["phase_nee"] > 0, a[3]
    assert stats_tuple(a[2]) == stats_tuple(b[2]) and a[3] == b[3]
    assert np.array_equal(a[0].view(u32), b[0].view(u32))


# ---- 3. physics ------------------------------------------------------------------------------------------------------
def _empty_scene(crt, lookfrom, vfov, w, h, lights=()):
    desc = crt.usda.SceneDesc()
    desc.camera = dict(lookfrom=lookfrom, lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=vfov, aspect=w / h, aperture=0.0, focus_dist=1.0)
    desc.settings.update(width=w, height=h, strategy="power")
    desc.lights = list(lights)
    return desc


def test_absorbing_slab_is_beer_lambert(crt, oracle, work, host):
    """Empty scene, sky only, a grey homogeneous region sigma_a = 0.7, sigma_s = 0, half extent 1 seen through a 1 degree
    lens: every camera ray crosses 2 units (within 1e-3: 2 / cos(0.5 deg) = 2.00008), survives delta tracking with
    probability e^-1.4 and then carries the sky. The frame mean of pixel / sky(direction) is a binomial estimate of
    p = e^-1.4 from N = 32 * 32 * 64 = 65 536 walks: within five standard errors sqrt(p (1 - p) / N)."""
    w = h = 32
    desc = _empty_scene(crt, (0.0, 0.0, -10.0), 1.0, w, h)
    o = ora_world.OracleRenderer(desc, crt.usda, max_depth=4)
    vol = crt.volumes.Volumes([crt.volumes.region(half_extent=1.0, sigma_a=0.7, sigma_s=0.0)])
    img, _counts, st, cov = vp.VolumeIntegrator(work, o, vp.host_table(host, vol.image_bytes())).render(64)
    assert st.camera_rays == w * h * 64 == st.ended_escaped and cov["phase_vertices"] == 0
    # sky(direction) of every pixel centre (tracer.rs:1334-1336); across one pixel of this lens it moves by < 1e-4 of itself
    cam = o.job.camera
    g = lambda v: np.array([v.x, v.y, v.z], np.float64)
    uu, vv = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    d = g(cam.lower_left)[None, None] + uu[None, :, None] * g(cam.horizontal)[None, None] + vv[:, None, None] * g(cam.vertical)[None, None] - g(cam.origin)[None, None]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    t = 0.5 * (d[..., 1] + 1.0)
    sky = (1.0 - t)[..., None] * np.ones(3) + t[..., None] * np.array([0.5, 0.7, 1.0])
    p = math.exp(-1.4)
    n = w * h * 64
    got = float((img.astype(np.float64) / sky).mean())
    bound = 5.0 * math.sqrt(p * (1.0 - p) / n)
    print("absorbing slab: mean %.6f, e^-1.4 %.6f, five standard errors %.6f" % (got, p, bound))
    assert abs(got - p) <= bound, (got, p, bound)


@pytest.mark.parametrize("strategy", ["power", "balance", "light", "bsdf"])
def test_white_furnace(crt, oracle, work, host, strategy):
    """No geometry, one uniform dome of radiance 1, a region with sigma_s = 1, sigma_a = 0, g = 0.3, half extent 1, depth
    64: nothing absorbs, so every pixel's expectation is 1 under every strategy. The frame mean of N >= 65 536 samples is
    within 0.01 of 1 — the tolerance the reference's own statistical volume tests use (volume.rs:583-673); the run's own
    five-sigma spread must lie inside it (if it did not, N would have to rise, never the tolerance)."""
    w = h = 32
    # N = 65 536; the light strategy takes every escape's share from the one NEE sample per vertex, and its five-sigma
    # spread at that N is 0.017 — so it gets N = 262 144 (0.0085), the tolerance stays
    spp = 256 if strategy == "light" else 64
    desc = _empty_scene(crt, (0.0, 0.0, -6.0), 10.0, w, h, lights=[crt.usda.dome_light((1.0, 1.0, 1.0))])
    desc.settings["strategy"] = strategy
    o = ora_world.OracleRenderer(desc, crt.usda, max_depth=64)
    vol = crt.volumes.Volumes([crt.volumes.region(half_extent=1.0, sigma_s=1.0, sigma_a=0.0, g=0.3)])
    img, _counts, st, cov = vp.VolumeIntegrator(work, o, vp.host_table(host, vol.image_bytes())).render(spp)
    assert cov["phase_vertices"] > w * h * spp // 2 and (cov["phase_nee"] > 0) == (strategy != "bsdf")
    assert cov["phase_prev_escapes"] > 0
    lum = img.astype(np.float64).mean(axis=2)
    mean = float(lum.mean())
    # pixel means are independent estimates of 1 from `spp` samples each: their spread gives the frame mean's standard error
    five_sigma = 5.0 * float(lum.std(ddof=1)) / math.sqrt(w * h)
    print("white furnace %s: mean %.5f, five sigma %.5f, %d phase vertices" % (strategy, mean, five_sigma, cov["phase_vertices"]))
    assert five_sigma <= 0.01, (strategy, five_sigma)
    assert abs(mean - 1.0) <= 0.01, (strategy, mean)


# ---- 4. the launch plan ------------------------------------------------------------------------------------------------
def test_every_plan_with_volumes_keeps_the_rules(tmp_path):
    """plan_launches over plan_sweep.cpp's grid, volumes off and on (tests/launch_plan/volume_sweep.cpp): with volumes
    always per stage, no tail, full camera paths, no root cull, no pipelined shade and no slim state, the VOL shade key,
    the two new kernels named (the shadow one only where the shadow stage runs), the traversal kernels those of the
    per-stage plan, the stats build refused; without, no volume form in any plan."""
    out = str(tmp_path / "volume_sweep")
    src = os.path.join(ROOT, "tests", "launch_plan", "volume_sweep.cpp")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    counts = dict(kv.split("=") for kv in run.stdout.split())
    assert int(counts["cases"]) > 10 ** 6 and int(counts["planned"]) > 0, counts
    assert counts["refused"] == counts["stats_refused"], counts  # volumes refuse the stats build and nothing else
    assert counts["vol_keys"] == "12", counts
    # the grid is plan_sweep.cpp's (tests/launch_plan/sweep_common.h, sweep_grid): the base sweep's figures, which
    # tests/test_launch_plan.py pins for its default tuple
    assert (int(counts["engines"]), int(counts["cases"])) == (120, 16312320), counts


# ---- 5. the ABI, no device --------------------------------------------------------------------------------------------
def test_set_volumes_is_declared_exported_and_checks_its_renderer(crt):
    assert crt.ABI_SYMBOLS_RENDER_VOLUMES == ["crt_renderer_set_volumes"] and hasattr(crt.lib(), "crt_renderer_set_volumes")
    header = open(os.path.join(ROOT, "include", "crt_render_volumes.h")).read()
    assert "int crt_renderer_set_volumes(CrtRenderer *r, CrtVolumes *v);" in header
    vol = crt.volumes.Volumes([crt.volumes.region()])
    assert crt.lib().crt_renderer_set_volumes(None, vol.h) == -1  # CRT_ERR_BAD_ARG
    assert crt.lib().crt_renderer_set_volumes(None, None) == -1
    vol.close()  # the caller's reference was the only one
