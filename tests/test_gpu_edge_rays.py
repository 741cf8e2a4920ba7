"""The edge corpus (tests/edge_rays.py) through the HIP traversal kernels: bit for bit the oracle's answers (geom_id,
prim_id, t, u, v, normal, front_face, occluded) through the batched queries, their _stats forms (every counter the
oracle keeps, the f64-fallback lanes included) and the single-ray entry points, on every engine instance the selector
can pick for the batched queries; the scene's traversal error word stays clear. The CPU side is tests/test_edge_rays.py.

Traversal counters are compared on the finite rays only: a NaN in a slab (a NaN or infinite ray) is dropped by v_max_f32
but kept by the reference's SSE max (ora_sse_max) when it is the second operand, so such a ray may visit other nodes —
it still finds nothing in the triangle scenes the corpus gives it (its edge functions are NaN), which the answers check."""
import ctypes as C

import numpy as np
import pytest

import edge_rays as er
import ora

pytestmark = pytest.mark.gpu

# engine instance -> (environment, expected crt_scene_engine_select fields). The batched queries have no four-wave
# direct-engine instance (CRT_WIDE=2 is the renderer's): with direct leaves they run the three-wave DIRECT engine.
ENGINES = {
    "flat6": ({"CRT_WIDE": "0", "CRT_POOL_STACK_RT": "6", "CRT_DIRECT_LEAVES": "0"}, {"wide": 0, "direct": 0, "lds_stack": 6}),
    "deep10": ({"CRT_WIDE": "0", "CRT_POOL_STACK_RT": "10", "CRT_DIRECT_LEAVES": "0"}, {"wide": 0, "direct": 0, "lds_stack": 10}),
    "wide": ({"CRT_WIDE": "1", "CRT_DIRECT_LEAVES": "0"}, {"wide": 1, "direct": 0}),
    "direct": ({"CRT_WIDE": "2", "CRT_DIRECT_LEAVES": "1"}, {"wide": 0, "direct": 1}),
}
STAT_FIELDS = ("queries", "nodes", "leaves", "packets", "prims")


def _mismatch(cs, ix, what, a, b):
    bad = np.nonzero(a != b)[0] if a.ndim == 1 else np.nonzero((a != b).any(axis=1))[0]
    return [(cs[ix[j]].label, what) for j in bad[:5]]


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", er.NAMES)
def test_edge_corpus_matches_the_oracle_bitwise(crt, monkeypatch, engine, name):
    import torch
    env, want = ENGINES[engine]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o_scene, _ok = er.build(ora, name)
    p_scene, _pk = er.build(crt, name)
    sel = p_scene.engine_select(-2)
    assert all(sel[k] == v for k, v in want.items()), (engine, sel)
    cs = er.cases(name)
    bad = []
    st_c, st_a = ora.TravStats(), ora.TravStats()
    ds_c, ds_a = crt.CrtTravStats(), crt.CrtTravStats()
    for (lo, hi), ix in er.groups(cs).items():
        fin = [i for i in ix if er.finite(cs[i])]
        for sub, counted in ((ix, False), (fin, True)):  # the plain forms on every ray, the _stats forms on finite ones
            if not sub:
                continue
            rays = er.rays8([cs[i] for i in sub])
            if counted:
                ora.lib().ora_set_trav_stats(C.byref(st_c))
                ora.lib().ora_set_trav_stats_any(C.byref(st_a))
            try:
                hf, ids, front = o_scene.intersect_n(rays, lo, hi)
                occ = o_scene.occluded_n(rays, lo, hi)
            finally:
                ora.lib().ora_set_trav_stats(None)
                ora.lib().ora_set_trav_stats_any(None)
            d_rays = crt.rays_to_device(rays)
            hits = crt.hits_to_host(p_scene.intersect_n(d_rays, lo, hi, stats=ds_c if counted else None))
            got_occ = p_scene.occluded_n(d_rays, lo, hi, stats=ds_a if counted else None).cpu().numpy()
            torch.cuda.synchronize()
            z = (ids[:, 0] != ora.INVALID_ID).astype(np.uint32)  # t, u, v, normal, front_face: hits only
            bad += _mismatch(cs, sub, "geom_id", hits["geom_id"], ids[:, 0])
            bad += _mismatch(cs, sub, "prim_id", hits["prim_id"], ids[:, 1])
            bad += _mismatch(cs, sub, "t", hits["t"].view(np.uint32) * z, hf[:, 0].view(np.uint32) * z)
            bad += _mismatch(cs, sub, "normal", hits["normal"].view(np.uint32) * z[:, None],
                             hf[:, 1:4].view(np.uint32) * z[:, None])
            bad += _mismatch(cs, sub, "u", hits["u"].view(np.uint32) * z, hf[:, 4].view(np.uint32) * z)
            bad += _mismatch(cs, sub, "v", hits["v"].view(np.uint32) * z, hf[:, 5].view(np.uint32) * z)
            bad += _mismatch(cs, sub, "front_face", hits["front_face"] * z, front.astype(np.uint32) * z)
            bad += _mismatch(cs, sub, "occluded", got_occ.astype(np.uint8), occ)
    p_scene.traversal_error()  # no launch on this scene overflowed a stack
    assert not bad, (engine, name, len(bad), bad[:8])
    for kind, dev, o in (("closest", ds_c, st_c), ("any", ds_a, st_a)):
        for f in STAT_FIELDS:
            assert list(getattr(dev, f)) == list(getattr(o, f)), (engine, name, kind, f, list(getattr(dev, f)), list(getattr(o, f)))
        assert int(dev.instance_descents) == int(o.instance_descents), (engine, name, kind)
        assert int(dev.phase_lanes[7]) == int(o.fallback_lanes), (engine, name, kind, "f64-fallback lanes",
                                                                  int(dev.phase_lanes[7]), int(o.fallback_lanes))
    assert int(ds_c.accepted_hits) == int(st_c.accepted_hits), (engine, name)
    if name != "degenerate":
        assert st_c.fallback_accepts > 100 and st_a.fallback_accepts > 100, (name, st_c.fallback_accepts, st_a.fallback_accepts)


@pytest.mark.parametrize("name", er.NAMES)
def test_edge_corpus_through_the_single_ray_entry_points(crt, name):
    """crt_intersect1 / crt_occluded1 on every fifth corpus ray (non-finite ones included): the oracle's answers."""
    o_scene, _ok = er.build(ora, name)
    p_scene, _pk = er.build(crt, name)
    bad = []
    for c in er.cases(name)[::5]:
        r = crt.Ray(c.o, c.d, float(c.time), c.mask)
        o = o_scene.intersect(ora.ray(c.o, c.d, float(c.time), c.mask), c.t_min, c.t_max)
        h = p_scene.intersect(r, c.t_min, c.t_max)
        if (o is None) != (h is None):
            bad.append((c.label, "hit"))
        elif o is not None:
            if (h.geom_id, h.prim_id) != (o.geom_id, o.prim_id):
                bad.append((c.label, "ids"))
            got = np.array([h.t, h.u, h.v] + list(h.normal), np.float32).view(np.uint32)
            want = np.array([o.t, o.u, o.v, o.normal.x, o.normal.y, o.normal.z], np.float32).view(np.uint32)
            if not np.array_equal(got, want) or bool(h.front_face) != bool(o.front_face):
                bad.append((c.label, "t/u/v/normal/front"))
        if bool(p_scene.occluded(r, c.t_min, c.t_max)) != o_scene.occluded(ora.ray(c.o, c.d, float(c.time), c.mask),
                                                                          c.t_min, c.t_max):
            bad.append((c.label, "occluded"))
    assert not bad, (name, len(bad), bad[:8])
