"""The scenes, rays and expected answers tests/test_gpu_cubic_curves.py runs, computed once and shared
(tests/test_cubic_curves.py checks on the CPU that they meet the brute-force query's condition)."""
import functools

import cubic_ref as cu
import gpu_curve_cases as gc

N_RAYS = 2048
SCENES = {
    # name -> (scene, number of rays, seed of its rays, shutter times of its rays)
    "one": (cu.scene_one, N_RAYS, 111, (0.0,)),
    "tuft": (cu.scene_tuft, N_RAYS, 212, (0.0,)),
    "mixed": (cu.scene_mixed, N_RAYS, 313, (0.0,)),
    "instanced": (cu.scene_instanced, N_RAYS, 414, (0.0, 0.37, 1.0)),
    "deep": (cu.scene_deep, 256, 515, (0.0,)),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


@functools.lru_cache(maxsize=None)
def rays(name):
    _make, n, seed, times = SCENES[name]
    r = cu.scene_rays(scene(name), n, seed, times)
    r.setflags(write=False)
    return r


_references = {}


def reference(ora, name, k):
    """The brute-force answers for scene `name` and t range cu.T_RANGES[k] (ora: the built oracle module, which answers
    for the floor's triangles), computed once."""
    if (name, k) not in _references:
        lo, hi = cu.T_RANGES[k]
        ref = scene(name).query(ora, rays(name), lo, hi)
        for v in ref.values():
            v.setflags(write=False)
        _references[(name, k)] = ref
    return _references[(name, k)]


# ---------------------------------------------------------------- the USD stage of tests/gpu_curve_cases.py, cubic prims decoded
def usd_stage(crt, tmp_path, cubic_curves=True):
    """-> (SceneDesc, warnings raised while loading) for gpu_curve_cases.USDA."""
    import warnings
    path = tmp_path / "curves.usda"
    path.write_text(gc.USDA)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        desc = crt.usda.load(str(path), 48, 32, cubic_curves=cubic_curves)
    return desc, [str(x.message) for x in w]


USD_RAYS = (1024, 404, (0.15, 0.85))  # count, seed, how far along a segment or a span the aimed half points


def usd_rays(ref_scene):
    """The rays of the imported stage: consecutive spans of one curve (and segments of a polyline) share an end sphere,
    where two of them answer the same t, so the aimed half points at their interiors."""
    n, seed, along = USD_RAYS
    return cu.scene_rays(ref_scene, n, seed, along=along, edge=False)


def ref_of_desc(desc):
    """The CubicRefScene of a SceneDesc made of meshes and instanced curve prototypes (segments, spans or both)."""
    s = cu.CubicRefScene()
    for g in desc.geoms:
        if g["kind"] == "mesh":
            s.triangles(g["verts"], g["idx"], g["mask"])
        else:
            proto = desc.protos[g["proto"]]
            assert g["kind"] == "instance" and ("segments" in proto or "spans" in proto), g["kind"]
            inner = cu.CubicRefScene()
            if "segments" in proto:  # round first (usd_import.rs:2150-2158)
                inner.curves(proto["segments"])
            if "spans" in proto:
                inner.cubic(proto["spans"])
            s.instance(inner, g["l2w"], g.get("l2w_end"), g["mask"])
    return s
