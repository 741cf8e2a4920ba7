"""The Tri4 packet step and the stored flat normals on the device (tests/packet_cases.py): mixed visibility masks in a
packet, several hits in one packet (ties, zero-normal lanes), smooth and flat normals side by side and under a nested
instance. Bit for bit the oracle's hits, normals and traversal counters through the batched queries on every engine
instance the selector can pick (the knob sets of tests/test_gpu_edge_rays.py), and the oracle's image and ray counts
through the renderer's four-wave kernels as a 64 x 36 render at 4 spp. The host side is tests/test_flat_normals.py."""
import ctypes as C

import numpy as np
import pytest

import ora
import packet_cases as pc

pytestmark = pytest.mark.gpu

ENGINES = {
    "flat6": ({"CRT_WIDE": "0", "CRT_POOL_STACK_RT": "6", "CRT_DIRECT_LEAVES": "0"}, {"wide": 0, "direct": 0, "lds_stack": 6}),
    "deep10": ({"CRT_WIDE": "0", "CRT_POOL_STACK_RT": "10", "CRT_DIRECT_LEAVES": "0"}, {"wide": 0, "direct": 0, "lds_stack": 10}),
    "wide": ({"CRT_WIDE": "1", "CRT_DIRECT_LEAVES": "0"}, {"wide": 1, "direct": 0}),
    "direct": ({"CRT_WIDE": "2", "CRT_DIRECT_LEAVES": "1"}, {"wide": 0, "direct": 1}),
}
STAT_FIELDS = ("queries", "nodes", "leaves", "packets", "prims")
T_MIN, T_MAX = 0.001, float("inf")

_REF = {}


class _NoMaterials:
    @staticmethod
    def fill_material(m, _d):
        return m


def _build_geometry(api, name, usda):
    """The case's scene through `api` (the oracle or the package) without materials: the batched queries need none."""
    return pc.World(_NoMaterials).build_world(pc.desc(usda, name), api, lambda: None)


def _reference(name, usda):
    """The oracle's answers and counters for the case's ray batches: computed once, shared by the engine instances."""
    if name not in _REF:
        o_scene, _om, o_keep = _build_geometry(ora, name, usda)
        out = []
        for mask, rays in pc.rays(name):
            st_c, st_a = ora.TravStats(), ora.TravStats()
            ora.lib().ora_set_trav_stats(C.byref(st_c))
            ora.lib().ora_set_trav_stats_any(C.byref(st_a))
            try:
                hf, ids, front = o_scene.intersect_n(rays, T_MIN, T_MAX)
                occ = o_scene.occluded_n(rays, T_MIN, T_MAX)
            finally:
                ora.lib().ora_set_trav_stats(None)
                ora.lib().ora_set_trav_stats_any(None)
            out.append(dict(mask=mask, rays=rays, hf=hf, ids=ids, front=front, occ=occ, st_c=st_c, st_a=st_a))
        _REF[name] = out
    return _REF[name]


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", pc.NAMES)
def test_packet_cases_match_the_oracle_bitwise(crt, monkeypatch, engine, name):
    import torch
    env, want = ENGINES[engine]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene, _m, _keep = _build_geometry(crt, name, crt.usda)
    sel = scene.engine_select(-2)
    assert all(sel[k] == v for k, v in want.items()), (engine, sel)
    for ref in _reference(name, crt.usda):
        rays, hf, ids = ref["rays"], ref["hf"], ref["ids"]
        what = (engine, name, ref["mask"])
        ds_c, ds_a = crt.CrtTravStats(), crt.CrtTravStats()
        d_rays = crt.rays_to_device(rays)
        hits = crt.hits_to_host(scene.intersect_n(d_rays, T_MIN, T_MAX, stats=ds_c))
        occ = scene.occluded_n(d_rays, T_MIN, T_MAX, stats=ds_a).cpu().numpy()
        plain = crt.hits_to_host(scene.intersect_n(d_rays, T_MIN, T_MAX))
        torch.cuda.synchronize()
        assert np.array_equal(plain.view(np.uint8), hits.view(np.uint8)), what
        hit = ids[:, 0] != ora.INVALID_ID
        assert np.array_equal(hits["geom_id"], ids[:, 0]) and np.array_equal(hits["prim_id"], ids[:, 1]), what
        assert np.array_equal(hits["t"][hit].view(np.uint32), hf[hit, 0].view(np.uint32)), what
        assert np.array_equal(hits["normal"][hit].view(np.uint32), hf[hit, 1:4].view(np.uint32)), what
        assert np.array_equal(hits["u"][hit].view(np.uint32), hf[hit, 4].view(np.uint32)), what
        assert np.array_equal(hits["v"][hit].view(np.uint32), hf[hit, 5].view(np.uint32)), what
        assert np.array_equal(hits["front_face"][hit], ref["front"][hit].astype(np.uint32)), what
        assert np.array_equal(occ.astype(np.uint8), ref["occ"]), what
        for kind, dev, o in (("closest", ds_c, ref["st_c"]), ("any", ds_a, ref["st_a"])):
            for f in STAT_FIELDS:
                assert list(getattr(dev, f)) == list(getattr(o, f)), (what, kind, f, list(getattr(dev, f)), list(getattr(o, f)))
            assert int(dev.instance_descents) == int(o.instance_descents), (what, kind)
            assert int(dev.phase_lanes[7]) == int(o.fallback_lanes), (what, kind, int(dev.phase_lanes[7]), int(o.fallback_lanes))
        assert int(ds_c.accepted_hits) == int(ref["st_c"].accepted_hits), what
        # what the case is built to reach
        if name == "masks":
            g = set(ids[hit, 0].tolist())
            assert (0 in g) == (ref["mask"] != pc.SHADOW) and (1 in g) == (ref["mask"] != pc.CAMERA), (what, g)
        if name == "stack":
            n = pc.stack_crossings(rays)
            for k in (1, 2, 3, 4):
                assert int((n == k).sum()) >= 8, (what, k)
            front_most = hits["t"][(n == 4) & (rays[:, 5] > 0)]
            assert len(front_most) and np.all(front_most == np.float32(1.0))  # z = -1 -> the triangle at z = 0
            tie = hit & (ids[:, 0] == 1)
            assert int(tie.sum()) >= 20 and np.all(ids[tie, 1] == 1)  # coincident: the later lane wins (bvh.rs:542)
            assert int(ref["st_c"].fallback_lanes) > 0
        if name == "normals":
            for gid in (0, 1, 2):
                assert int((ids[hit, 0] == gid).sum()) > 60, (what, gid)
    scene.traversal_error()


@pytest.mark.parametrize("name", pc.NAMES)
def test_packet_cases_render_identically_on_the_four_wave_kernels(crt, monkeypatch, name):
    import torch
    import ora_world
    for k in ("CRT_FUSED", "CRT_STAGE_MIN_PATHS", "CRT_LANES", "CRT_LANE_MIN_PATHS", "CRT_WIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in {"CRT_FUSED": "0", "CRT_STAGE_MIN_PATHS": "1", "CRT_WIDE": "1"}.items():
        monkeypatch.setenv(k, v)
    desc = pc.desc(crt.usda, name)
    world = pc.World(crt.usda)
    scene, mats, _protos = world.build_world(desc, crt, crt.default_material)
    s = desc.settings
    settings = crt.RenderSettings(s["width"], s["height"], s["max_depth"], s["frame"], s["strategy"], s["filter"],
                                  s["filter_radius"], 0.0)
    r = crt.Renderer(scene, mats, desc.lights, crt.make_camera(**desc.camera), settings)
    r.render_samples(0, 4)
    torch.cuda.synchronize()
    img, st, pipe = r.image(), r.stats(), r.pipeline()
    scene.traversal_error()
    assert pipe["wide"] and not pipe["fused"], pipe
    oimg, ost = ora_world.OracleRenderer(desc, world).render(4, forward=1)
    for f, _t in ora.RayStats._fields_:
        assert getattr(st, f) == getattr(ost, f), (name, f, getattr(st, f), getattr(ost, f))
    assert st.camera_rays == 64 * 36 * 4 and st.shadow_rays > 0 and st.closest_hit > st.camera_rays
    assert np.isfinite(oimg).all() and len(np.unique(oimg.view(np.uint32))) > 500  # a picture, not a constant
    bad = np.argwhere(img.view(np.uint32) != oimg.view(np.uint32))
    assert bad.shape[0] == 0, (name, bad.shape[0], bad[:3])
