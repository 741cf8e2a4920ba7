"""BasisCurves through the USD reader (crust-render_amd/usda.py; usd_import.rs:1993-2093, :2133-2170): linear curves become
round curve segments in a scene of their own under ONE instance; cubic ones are named and skipped. Runs without a GPU;
the queries on the imported scene are in tests/test_gpu_curves.py."""
import numpy as np

import gpu_curve_cases as gc

f32 = np.float32


def test_linear_basis_curves_become_instanced_segments(crt, tmp_path):
    desc, warned = gc.usd_stage(crt, tmp_path)
    names = [g["name"] for g in desc.geoms]
    assert names.count("Tripod") == 1 and names.count("Polyline") == 1  # one instance per prim
    assert "Tuft" not in names and "Flattened" not in names             # cubic: skipped; non-invertible: skipped
    assert len([w for w in warned if "Tuft" in w and "cubic" in w]) == 1, warned
    assert not [w for w in warned if "Tripod" in w or "Polyline" in w], warned
    by = {g["name"]: g for g in desc.geoms}
    tri, poly = by["Tripod"], by["Polyline"]
    assert tri["kind"] == "instance" and poly["kind"] == "instance" and by["Floor"]["kind"] == "mesh"
    st, sp = desc.protos[tri["proto"]]["segments"], desc.protos[poly["proto"]]["segments"]
    assert st.shape == (3, 8) and st.dtype == np.float32
    assert np.all(st[:, 3] == f32(0.5) * f32(0.07)) and np.all(st[:, 7] == f32(0.5) * f32(0.07))  # constant width: r = w / 2
    assert np.array_equal(st[:, 0:3], np.array([(0.5, 0, 0.1), (-0.3, 0, 0.45), (-0.2, 0, -0.5)], np.float32))  # local space
    assert np.array_equal(st[:, 4:7], np.array([(0, 1.2, 0)] * 3, np.float32))  # three two-point curves: no segment between them
    # the placement is the prim's world transform: translate * scale
    assert np.array_equal(tri["l2w"], np.array([1.25, 0, 0, 0, 1.5, 0, 0, 0, 0.75, 1, 0, -0.75], np.float32))
    # per-vertex widths; the third curve's count (6) overruns the eight points: the prim stops there
    assert sp.shape == (4, 8)
    assert np.array_equal(sp[1:3, 0:3], sp[0:2, 4:7]) and not np.array_equal(sp[3, 0:3], sp[2, 4:7])
    w = np.array([0.24, 0.18, 0.1, 0.05, 0.28, 0.09], np.float32) * f32(0.5)
    assert np.array_equal(sp[:, 3], w[[0, 1, 2, 4]]) and np.array_equal(sp[:, 7], w[[1, 2, 3, 5]])
    # the prim's bound material arrives on the instance's geometry entry; an unbound prim gets the default, as the floor
    assert poly["material"]["_path"] == "/Stage/Looks/Straw"
    assert tuple(f32(x) for x in poly["material"]["base_color"]) == (f32(0.62), f32(0.48), f32(0.21))
    assert f32(poly["material"]["specular_roughness"]) == f32(0.45)
    assert tri["material"] == by["Floor"]["material"] and "_path" not in tri["material"]


def test_width_interpolation_is_resolved_from_the_array_length(crt):
    class P:
        path = "/P"

        def __init__(self, **a):
            self.attrs = a

        def attr(self, n, d=None):
            return self.attrs.get(n, d)
    pts = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 0)]
    seg = crt.usda._linear_curve_segments
    per_curve = seg(P(points=pts, curveVertexCounts=[3, 2], widths=[0.4, 0.2]))
    assert per_curve[:, 3].tolist() == [f32(0.2), f32(0.2), f32(0.1)] and per_curve[:, 7].tolist() == [f32(0.2), f32(0.2), f32(0.1)]
    first = seg(P(points=pts, curveVertexCounts=[3, 2], widths=[0.4, 0.2, 0.1]))  # neither per vertex nor per curve
    assert set(first[:, 3].tolist()) == {f32(0.2)}
    none = seg(P(points=pts, curveVertexCounts=[3, 2]))  # no widths: 1.0
    assert set(none[:, 7].tolist()) == {f32(0.5)}
    hair = seg(P(points=pts, curveVertexCounts=[3, 2], widths=[0.0]))
    assert set(hair[:, 3].tolist()) == {f32(0.5) * f32(1e-6)}
    assert seg(P(points=pts)) is None and seg(P(curveVertexCounts=[2])) is None
    assert seg(P(points=pts, curveVertexCounts=[3, 2], basis="hermite")) is None
    assert seg(P(points=pts, curveVertexCounts=[1, 1, 3])).shape == (2, 8)  # single points make no segment
    # no segment at all: nothing is emitted (no geometry id, no material slot), usd_import.rs:2118-2121
    assert seg(P(points=pts, curveVertexCounts=[1, 1, 1])) is None and seg(P(points=pts, curveVertexCounts=[6, 2])) is None


def test_imported_curve_scene_builds(crt, tmp_path):
    desc, _ = gc.usd_stage(crt, tmp_path)
    scene, mats, protos = crt.usda.build_world(desc, crt, crt.default_material)
    assert len(mats) == len(desc.geoms) == scene.geometry_count()
    bd = scene.unique_primitive_breakdown()
    assert bd["curve_segments"] == 7 and bd["instances"] == 2 and bd["triangles"] == 2, bd
    assert scene.image_check()["instances"] == 2
    sel = scene.engine_select(-3)
    assert sel["wide"] == 0 and sel["cold"] & 16, sel
    assert gc.ref_of_desc(desc).n_segments() == 7


def test_undecided_rays_of_the_imported_stage_stay_under_the_cap(crt, oracle, tmp_path):
    """Condition on the rays tests/test_gpu_curves.py sends through the imported scene: at most 1 % of them undecided
    under the brute-force query, and enough of them meet a curve for the comparison to say something."""
    import curve_ref as cr
    desc, _ = gc.usd_stage(crt, tmp_path)
    ref_scene = gc.ref_of_desc(desc)
    ref = ref_scene.query(oracle, gc.usd_rays(ref_scene), 0.001, float("inf"))
    und = float((~ref["decided"]).mean())
    on_curves = int((ref["hit"] & (ref["geom"] != len(desc.geoms) - 1)).sum())
    print("usd: undecided %.4f (%d of %d), on curves %d" % (und, int((~ref["decided"]).sum()), len(ref["decided"]), on_curves))
    assert und <= cr.UNDECIDED_CAP, und
    assert on_curves > 50


def test_curves_inside_a_prototype_are_named_and_skipped(crt, tmp_path):
    """A BasisCurves prim reached through a PointInstancer's prototype is not decoded yet: the reader says so."""
    import warnings
    path = tmp_path / "instanced_curves.usda"
    path.write_text('''#usda 1.0
(
    defaultPrim = "Stage"
)
def Xform "Stage"
{
    def Camera "Eye"
    {
        double3 xformOp:translate = (0, 1, 6)
        uniform token[] xformOpOrder = ["xformOp:translate"]
    }
    def PointInstancer "Field"
    {
        rel prototypes = [</Stage/Field/Protos/Blade>]
        int[] protoIndices = [0, 0]
        point3f[] positions = [(-1, 0, 0), (1, 0, 0)]
        def Scope "Protos"
        {
            def Xform "Blade"
            {
                def BasisCurves "Stem"
                {
                    uniform token type = "linear"
                    int[] curveVertexCounts = [2]
                    point3f[] points = [(0, 0, 0), (0.1, 0.9, 0)]
                    float[] widths = [0.06]
                }
                def Mesh "Leaf"
                {
                    int[] faceVertexCounts = [3]
                    int[] faceVertexIndices = [0, 1, 2]
                    point3f[] points = [(0, 0.4, 0), (0.3, 0.5, 0), (0, 0.6, 0.1)]
                }
            }
        }
    }
}
''')
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        desc = crt.usda.load(str(path), 48, 32)
    assert len([x for x in w if "/Stage/Field/Protos/Blade/Stem" in str(x.message) and "prototype" in str(x.message)]) == 1, [str(x.message) for x in w]
    assert len(desc.geoms) == 2 and all(g["kind"] == "instance" for g in desc.geoms)  # the leaf, twice
