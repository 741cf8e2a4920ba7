"""Environment-mapped dome lights on the GPU: the exported light functions against the float32 restatement
(tests/env_ref.py), the id table, and renders of mapped domes against the reference's integrator run on the device's seam
functions (tests/seam_integrator.py) — the oracle knows no mapped dome, its light table holds a uniform dome at that index
and every light call goes through the hooks. The CPU half is tests/test_environment.py."""
import ctypes as C
import os

import numpy as np
import pytest

import env_cases as ec
import env_ref as er
import ora
import ora_world
import seam_cases as sc
import seam_integrator as si

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
PAIRS = [("hand_8x4", "sky_env_rotY20"), ("3x2", "spotty_64x32"), ("black_8x4", "skewed_3x2"), ("1x1", "uniform_32x16"),
         ("sky_env", "spotty_32x16"), ("uniform_64x32", "hand_8x4")]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return er.host(tmp_path_factory.mktemp("env_host"))


@pytest.fixture(scope="module")
def maps(crt):
    return ec.maps(crt)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and bool(np.all((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))))


def _mapped_record(crt, env, tint):
    l = crt.CrtLight()
    t = np.asarray(tint, dtype=f32)
    assert crt.lib().crt_light_dome_mapped(C.byref(l), t.ctypes.data_as(C.POINTER(C.c_float)), env.h) == 0
    return np.frombuffer(bytes(l), dtype=sc.LIGHT)[0]


# ---- 8. the seam functions == the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_light_functions_equal_the_restatement(crt, oracle, H, maps, pair):
    """One light table: sphere, rect, distant and uniform-dome lights and mapped domes over two environments.
    crt_light_sample_n / _escaped_n / _pdf_n: the mapped domes == tests/env_ref.py bit for bit (100 000 seeded calls plus
    the edge list per map), the four old kinds == the oracle's functions through the same launches."""
    import torch
    rng = np.random.default_rng(sum(map(ord, "".join(pair))))
    old = sc.lights(rng, 2)
    envs = [crt.Environment(*maps[name]) for name in pair]
    refs = [er.EnvRef(H, *maps[name]) for name in pair]
    tints = [ec.TINT, np.array([0.5, 1.0, 0.25], dtype=f32)]
    table = np.concatenate([old, np.array([_mapped_record(crt, e, t) for e, t in zip(envs, tints)], dtype=sc.LIGHT)])
    assert list(table["kind"][-2:]) == [4, 4]
    dl = crt.shading.DeviceLights((crt.CrtLight * len(table)).from_buffer_copy(table.tobytes()))
    drv = sc.oracle_drivers()

    # the old kinds: random queries over the whole table, old and mapped records in the same launches
    n = 100_000
    q = sc.light_queries(20_000, table, rng)
    d_q = crt.shading.to_device(q)
    got_s, got_e = _host(dl.sample_li(d_q), sc.LIGHT_SAMPLE), _host(dl.escaped(d_q), sc.LIGHT_SAMPLE)
    got_p = _host(dl.pdf_at_point(d_q), f32)
    torch.cuda.synchronize()
    is_old = q["light"] < len(old)
    assert len(sc.mismatches(got_s[is_old], drv.light_sample(old, q[is_old]))) == 0
    assert len(sc.mismatches(got_e[is_old], drv.light_escaped(old, q[is_old]))) == 0
    assert same_bits(got_p[is_old], drv.light_pdf(old, q[is_old]))
    assert (got_p[~is_old] == 0).all()  # the trait's default for lights at infinity

    for k, (R, tint, name) in enumerate(zip(refs, tints, pair)):
        eu, ev = ec.edge_uv(R)
        ed = ec.edge_directions(R)
        m = n + max(len(eu), len(ed))
        q = np.zeros(m, dtype=sc.LIGHT_QUERY)
        q["light"] = len(old) + k
        q["from"] = rng.uniform(-6, 6, size=(m, 3)).astype(f32)
        q["u"], q["v"] = rng.random(m, dtype=f32), rng.random(m, dtype=f32)
        q["u"][n:n + len(eu)], q["v"][n:n + len(ev)] = eu, ev
        q["point"] = ec.random_directions(rng, m)
        q["point"][n:n + len(ed)] = ed
        d_q = crt.shading.to_device(q)
        s, e = _host(dl.sample_li(d_q), sc.LIGHT_SAMPLE), _host(dl.escaped(d_q), sc.LIGHT_SAMPLE)
        p = _host(dl.pdf_at_point(d_q), f32)
        torch.cuda.synchronize()
        wd, wr, wp, wsome = R.light_sample(tint, q["u"], q["v"])
        assert np.array_equal(s["some"] != 0, wsome), (name, "sample some")
        assert same_bits(s["direction"], wd) and same_bits(s["radiance"], wr) and same_bits(s["pdf"], wp), (name, "sample")
        assert np.isinf(s["distance"][wsome]).all() and (s["distance"][~wsome] == 0).all(), name
        er_, ep = R.light_escaped(tint, q["point"])
        assert (e["some"] == 1).all() and same_bits(e["radiance"], er_) and same_bits(e["pdf"], ep), (name, "escaped")
        assert same_bits(e["direction"], q["point"]) and (p == 0).all(), name
        if name.startswith("black"):
            assert not wsome.any()
        else:
            assert wsome[:n].mean() > 0.99, name


# ---- 9. ids ------------------------------------------------------------------------------------------------------------------
def _render_args(crt):
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "cornellbox.usda"), 16, 16)
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], 4, s["frame"], s["strategy"], s["filter"], s["filter_radius"], 0.0)
    return scene, mats, crt.make_camera(**desc.camera), settings, protos


def test_ids_that_name_no_environment_answer_none(crt, maps):
    import torch
    keep = crt.Environment(*maps["3x2"])       # a live environment: the launches take the instance with the mapped arm
    gone = crt.Environment(*maps["hand_8x4"])
    live, freed = _mapped_record(crt, keep, ec.TINT), _mapped_record(crt, gone, ec.TINT)
    table = np.array([live, freed, live, live, live], dtype=sc.LIGHT)
    words = table.view(u32).reshape(len(table), sc.LIGHT.itemsize // 4)  # the id's bits are written as bits: word 5 = center[0]
    assert sc.LIGHT.fields["center"][1] == 20
    live_id = int(words[0, 5])
    assert live_id == keep.tables()["id"]
    words[2, 5] = 0xFFFFFFF0 | 5    # a slot nothing lives in, a generation never handed out
    words[3, 5] = 0                 # generation 0 names nothing
    words[4, 5] = live_id + 16      # the live slot, another generation
    q = np.zeros(5 * 64, dtype=sc.LIGHT_QUERY)
    q["light"] = np.repeat(np.arange(5, dtype=u32), 64)
    rng = np.random.default_rng(1)
    q["u"], q["v"], q["point"] = rng.random(len(q), dtype=f32), rng.random(len(q), dtype=f32), ec.random_directions(rng, len(q))
    dl = crt.shading.DeviceLights((crt.CrtLight * len(table)).from_buffer_copy(table.tobytes()))
    d_q = crt.shading.to_device(q)
    s = _host(dl.sample_li(d_q), sc.LIGHT_SAMPLE)
    torch.cuda.synchronize()
    assert s["some"][:128].all() and not s["some"][128:].any()  # both environments live: two records answer
    torch.cuda.synchronize()  # the streams are drained: nothing reads the environment about to go
    gone.free()
    s, e = _host(dl.sample_li(d_q), sc.LIGHT_SAMPLE), _host(dl.escaped(d_q), sc.LIGHT_SAMPLE)
    torch.cuda.synchronize()
    for got in (s, e):
        assert got["some"][:64].all() and not got["some"][64:].any()
        assert (got["radiance"][64:] == 0).all() and (got["pdf"][64:] == 0).all()

    scene, mats, cam, settings, _protos = _render_args(crt)
    cs = settings.c()
    marr = (crt.CrtMaterial * len(mats))(*mats)
    for k, why in ((1, "freed"), (2, "out of range"), (3, "zero"), (4, "older generation")):
        arr = (crt.CrtLight * 1).from_buffer_copy(table[k:k + 1].tobytes())
        h = crt.lib().crt_renderer_new(scene.h, marr, len(mats), arr, 1, C.byref(cam), C.byref(cs), 0, 1)
        assert not h, why
        assert b"not live" in crt.lib().crt_last_error(), why
    arr = (crt.CrtLight * 1).from_buffer_copy(table[0:1].tobytes())
    h = crt.lib().crt_renderer_new(scene.h, marr, len(mats), arr, 1, C.byref(cam), C.byref(cs), 0, 1)
    assert h
    keep.free()  # the renderer retains the environment its light names
    assert crt.lib().crt_render_samples(h, 0, 1, None) == 0
    torch.cuda.synchronize()
    crt.lib().crt_renderer_free(h)


# ---- 10, 12. renders == the reference's integrator on the device's seam functions ---------------------------------------
def _check_render(crt, desc, spp, name, want_class=None):
    """The device's wavefront render of `desc` against the oracle's trace_path hooked onto crt_intersect1 / crt_occluded1
    and the six seam functions, both estimator orders."""
    import torch
    scene, mats, _protos = crt.usda.build_world(desc, crt, crt.default_material)
    o = ora_world.OracleRenderer(desc, crt.usda)  # its own light table: a uniform dome where ours is mapped
    host = si.SeamHost(si.DeviceKernel(crt, scene), si.DeviceShade(crt, mats, desc.lights))
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"], s["frame"], s["strategy"], s["filter"],
                                  s["filter_radius"], 0.0)
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r.render_samples(0, spp)
    torch.cuda.synchronize()
    dimg, dst = r.image(), r.stats()
    assert not r.pipeline()["fused"], name  # lights at infinity never run the fused kernel
    img, st = host.render(o, spp, 1)
    assert host.calls["escaped"] > 0, (name, host.calls)
    assert host.calls["sample_li"] > 0 or s["strategy"] == "bsdf", (name, host.calls)  # the bsdf strategy samples no light
    for f, _t in ora.RayStats._fields_:
        assert getattr(dst, f) == getattr(st, f), (name, f, getattr(dst, f), getattr(st, f))
    bad = np.argwhere(dimg.view(u32) != img.view(u32))
    assert bad.shape[0] == 0, (name, bad.shape[0], bad[:3])
    ref, st0 = host.render(o, spp, 0)  # the reference-order (backward gather) estimator
    for f, _t in ora.RayStats._fields_:
        assert getattr(dst, f) == getattr(st0, f), (name, f)
    err = np.abs(dimg - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= 1e-5, (name, err.max())  # the tolerance of test_forward_equals_reference_gather_within_float_association
    if want_class is not None:  # the look that selects the kernel instance is in the table the renderer was given
        def cls(m):  # launch_plan.h, material_class
            if m.kind == crt.MAT_EMISSIVE:
                return 0
            if m.transmission_weight > 0 or m.subsurface_weight > 0:
                return 3
            return 2 if (m.coat_weight > 0 or m.fuzz_weight > 0 or m.thin_film_weight > 0) else 1
        assert max(cls(m) for m in mats) == want_class, (name, [cls(m) for m in mats])
    return dimg


def test_domelight_render_equals_the_hooked_reference_integrator(crt, oracle):
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "domelight.usda"), 40, 24, environment_maps=True)
    desc.settings["max_depth"] = 8
    assert "environment" in [l for l in desc.lights if l["kind"] == "dome"][0]
    img = _check_render(crt, desc, 2, "domelight")
    assert np.isfinite(img).all() and img.max() > 0


# Which shade instance a light list with a mapped dome runs follows from the material table (launch_plan.h, plan_launches: the k_shade_env rows):
# simple materials k_shade_env<0, true> (derived records, the default) or <0, false> (CRT_MAT_DERIVED=0); any coat, fuzz or
# thin-film material <1, false>; any material with an interior medium <2, false>. domelight itself is all simple, so each
# of the other three is reached by changing one look of that scene.
VARIANTS = {
    "raw_records": (dict(), {"CRT_MAT_DERIVED": "0"}, 1),
    "general_by_knob": (dict(), {"CRT_SIMPLE": "0"}, 1),
    "coat_and_fuzz": (dict(Matte=dict(coat_weight=0.8, coat_roughness=0.1, coat_color=(0.9, 0.8, 0.7), fuzz_weight=0.4,
                                      fuzz_roughness=0.5)), {}, 2),
    "thin_film": (dict(Chrome=dict(thin_film_weight=1.0, thin_film_thickness=0.45)), {}, 2),
    "glass_with_medium": (dict(Chrome=dict(base_metalness=0.0, transmission_weight=1.0, transmission_color=(0.7, 0.9, 0.8),
                                           transmission_depth=0.6, specular_roughness=0.05)), {}, 3),
    "subsurface": (dict(Matte=dict(subsurface_weight=0.9, subsurface_color=(0.8, 0.5, 0.4), subsurface_radius=0.3)), {}, 3),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_mapped_dome_shade_instance_equals_the_hooked_reference_integrator(crt, oracle, monkeypatch, variant):
    """The parity of the domelight render on every kernel instance crt_render_samples can pick for a light list that holds
    a mapped dome: image bits and all eight counters against the oracle's trace_path on the device's seam functions."""
    looks, env, want_class = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "domelight.usda"), 40, 24, environment_maps=True)
    desc.settings["max_depth"] = 8
    for g in desc.geoms:
        if g["name"] in looks:
            g["material"] = dict(g["material"], **looks[g["name"]])
    assert not looks or sum(g["name"] in looks for g in desc.geoms) == len(looks)
    img = _check_render(crt, desc, 2, "domelight/" + variant, want_class)
    assert np.isfinite(img).all() and img.max() > 0


@pytest.mark.parametrize("strategy", ["power", "balance", "light", "bsdf"])
def test_mixed_lights_render_equals_the_hooked_reference_integrator(crt, oracle, maps, strategy):
    """Two mapped domes over different environments, a rect light and a sphere light in one hand-built scene."""
    desc = crt.usda.load(os.path.join(ROOT, "scenes", "veach_mis.usda"), 32, 32)
    desc.settings["max_depth"] = 6
    desc.settings["strategy"] = strategy
    kinds = [l["kind"] for l in desc.lights]
    assert "sphere" in kinds
    if "rect" not in kinds:  # a rect light over the plates, with the emissive quad it samples
        origin, eu, ev = np.array([-1.0, 6.0, -1.0], f32), np.array([2.0, 0, 0], f32), np.array([0, 0, 2.0], f32)
        verts = np.stack([origin, origin + eu, origin + eu + ev, origin + ev]).astype(f32)
        rad = np.array([6.0, 5.0, 4.0], f32)
        gid = len(desc.geoms)
        desc.geoms.append(dict(kind="mesh", verts=verts, idx=np.array([(0, 1, 2), (0, 2, 3)], u32), mask=0xFFFFFFFF,
                               material={"_preset": "emissive", "emission_color": tuple(rad)}, name="Rect"))
        desc.lights.append(dict(kind="rect", geom_id=gid, radiance=rad, origin=origin, edge_u=eu, edge_v=ev,
                                normal=np.array([0, -1.0, 0], f32)))
    for name, tint in (("sky_env_rotY20", (0.6, 0.6, 0.6)), ("hand_8x4", (0.2, 0.3, 0.4))):
        w, h, rgb, m = maps[name]
        desc.lights.append(crt.usda.dome_light(tint, dict(width=w, height=h, rgb=rgb, light_to_world=m)))
    assert sorted(set(l["kind"] for l in desc.lights)) == ["dome", "rect", "sphere"]
    _check_render(crt, desc, 2, "mixed/" + strategy)


# ---- 11. pipelines and determinism ---------------------------------------------------------------------------------------
def _domelight(crt, environment_maps=True):
    import torch
    r, desc = crt.load_usda(os.path.join(ROOT, "scenes", "domelight.usda"), 96, 54, 8, environment_maps=environment_maps)
    return r, torch


def test_domelight_lanes_batches_and_runs_agree(crt, monkeypatch):
    monkeypatch.setenv("CRT_LANES", "1")
    one, torch = _domelight(crt)
    one.render_samples(0, 8)
    torch.cuda.synchronize()
    base = one.image().copy()
    assert one.lanes() == 1 and one.pipeline()["fused"] is False  # a per-stage pipeline: mapped domes are lights at infinity
    for _ in range(2):  # three runs in one process give identical bits
        one.clear()
        one.render_samples(0, 8)
        torch.cuda.synchronize()
        assert np.array_equal(one.image().view(u32), base.view(u32))
    one.clear()
    one.render_samples(0, 4)  # one batch == two half batches
    one.render_samples(4, 4)
    torch.cuda.synchronize()
    assert np.array_equal(one.image().view(u32), base.view(u32))
    monkeypatch.setenv("CRT_LANES", "3")
    monkeypatch.setenv("CRT_LANE_MIN_PATHS", "1")
    three, _ = _domelight(crt)
    three.render_samples(0, 8)
    torch.cuda.synchronize()
    assert three.lanes() == 3
    assert np.array_equal(three.image().view(u32), base.view(u32))  # one lane == three lanes
    with pytest.warns(UserWarning, match="not decoded"):
        uniform, _ = _domelight(crt, environment_maps=False)
    uniform.render_samples(0, 8)
    torch.cuda.synchronize()
    assert np.isfinite(base).all()
    assert not np.array_equal(uniform.image().view(u32), base.view(u32))  # the map is in the picture
