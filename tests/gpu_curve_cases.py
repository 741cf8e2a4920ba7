"""The scenes, rays and expected answers tests/test_gpu_curves.py runs, computed once and shared (tests/test_curves.py
checks on the CPU that they meet the brute-force query's condition)."""
import functools

import curve_ref as cr

N_RAYS = 4096
SCENES = {
    # name -> (scene, seed of its rays, shutter times of its rays)
    "one": (cr.scene_one, 101, (0.0,)),
    "tuft": (cr.scene_tuft, 202, (0.0,)),
    "instanced": (cr.scene_instanced, 303, (0.0, 0.37, 1.0)),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


@functools.lru_cache(maxsize=None)
def rays(name):
    _make, seed, times = SCENES[name]
    r = cr.scene_rays(scene(name), N_RAYS, seed, times)
    r.setflags(write=False)
    return r


_references = {}


def reference(ora, name, k):
    """The brute-force answers for scene `name` and t range cr.T_RANGES[k] (ora: the built oracle module, which answers
    for the floor's triangles), computed once."""
    if (name, k) not in _references:
        lo, hi = cr.T_RANGES[k]
        ref = scene(name).query(ora, rays(name), lo, hi)
        for v in ref.values():
            v.setflags(write=False)
        _references[(name, k)] = ref
    return _references[(name, k)]


# ---------------------------------------------------------------- a USD stage with curves, written here
USDA = '''#usda 1.0
(
    defaultPrim = "Stage"
    upAxis = "Y"
)

def Xform "Stage"
{
    def Camera "Eye"
    {
        float focalLength = 35
        float horizontalAperture = 24
        double3 xformOp:translate = (0.5, 1.5, 7)
        uniform token[] xformOpOrder = ["xformOp:translate"]
    }

    def Scope "Looks"
    {
        def Material "Straw"
        {
            token outputs:surface.connect = </Stage/Looks/Straw/Surface.outputs:surface>
            def Shader "Surface"
            {
                uniform token info:id = "crust:openpbr"
                color3f inputs:baseColor = (0.62, 0.48, 0.21)
                float inputs:specularRoughness = 0.45
                token outputs:surface
            }
        }
    }

    def BasisCurves "Tuft"
    {
        uniform token type = "cubic"
        uniform token basis = "bspline"
        int[] curveVertexCounts = [5]
        point3f[] points = [(3.1, 0, 1.2), (3.3, 0.5, 1.1), (3.0, 0.9, 1.4), (3.4, 1.3, 1.2), (3.2, 1.6, 1.5)]
        float[] widths = [0.09] (
            interpolation = "constant"
        )
    }

    def BasisCurves "Tripod"
    {
        uniform token type = "linear"
        int[] curveVertexCounts = [2, 2, 2]
        point3f[] points = [(0.5, 0, 0.1), (0, 1.2, 0), (-0.3, 0, 0.45), (0, 1.2, 0), (-0.2, 0, -0.5), (0, 1.2, 0)]
        float[] widths = [0.07] (
            interpolation = "constant"
        )
        double3 xformOp:translate = (1, 0, -0.75)
        float3 xformOp:scale = (1.25, 1.5, 0.75)
        uniform token[] xformOpOrder = ["xformOp:translate", "xformOp:scale"]
    }

    def BasisCurves "Polyline" (prepend apiSchemas = ["MaterialBindingAPI"])
    {
        rel material:binding = </Stage/Looks/Straw>
        uniform token type = "linear"
        int[] curveVertexCounts = [4, 2, 6]
        point3f[] points = [(-2.4, 0, 0.3), (-2.2, 0.6, 0.5), (-2.5, 1.1, 0.2), (-2.1, 1.6, 0.4),
                            (-0.9, 0, -0.6), (-0.7, 0.9, -0.8), (0.2, 0, 1.3), (0.3, 0.8, 1.2)]
        float[] widths = [0.24, 0.18, 0.1, 0.05, 0.28, 0.09, 0.14, 0.03] (
            interpolation = "vertex"
        )
    }

    def BasisCurves "Flattened"
    {
        uniform token type = "linear"
        int[] curveVertexCounts = [2]
        point3f[] points = [(2, 0, 2), (2, 1, 2.5)]
        float[] widths = [0.4]
        float3 xformOp:scale = (1, 1, 0)
        uniform token[] xformOpOrder = ["xformOp:scale"]
    }

    def Mesh "Floor"
    {
        int[] faceVertexCounts = [4]
        int[] faceVertexIndices = [0, 1, 2, 3]
        point3f[] points = [(-7, 0, -7), (7, 0, -7), (7, 0, 7), (-7, 0, 7)]
    }
}
'''


def usd_stage(crt, tmp_path):
    """-> (SceneDesc, warnings raised while loading) for USDA above."""
    import warnings
    path = tmp_path / "curves.usda"
    path.write_text(USDA)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        desc = crt.usda.load(str(path), 48, 32)
    return desc, [str(x.message) for x in w]


USD_RAYS = (1024, 404, (0.15, 0.85))  # count, seed, how far along a segment's axis the aimed half points


def usd_rays(ref_scene):
    """The rays of the imported stage. Its prims are polylines: consecutive segments share an end sphere, where two
    segments answer the same t, so the aimed half points at the segments' bodies, not at their ends."""
    n, seed, along = USD_RAYS
    return cr.scene_rays(ref_scene, n, seed, along=along)


def ref_of_desc(desc):
    """The RefScene of a SceneDesc made of meshes and instanced curve prototypes."""
    s = cr.RefScene()
    for g in desc.geoms:
        if g["kind"] == "mesh":
            s.triangles(g["verts"], g["idx"], g["mask"])
        else:
            assert g["kind"] == "instance" and "segments" in desc.protos[g["proto"]], g["kind"]
            inner = cr.RefScene()
            inner.curves(desc.protos[g["proto"]]["segments"])
            s.instance(inner, g["l2w"], g.get("l2w_end"), g["mask"])
    return s
