"""Per-face textures on the GPU (include/crt_face_textures.h), function by function and bit for bit against
tests/face_ref.py and the oracle's untextured material functions: crt_face_resolve_n on hits crt_intersect_n wrote over a
scene of quads, triangles, a pentagon, a mirrored copy, an instanced mesh and a sphere; crt_face_texture_eval_n over
textures from 1x1 to 64x16 with the refusal inputs; crt_material_scatter_faces_n / _eval_faces_n per lobe class against
the untextured functions on the substituted table. The counts are no multiple of the 256-lane block."""
import numpy as np
import pytest

import face_cases as fc
import face_ref as fr
import seam_cases as sc

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
N = 10037
N_SHADE = 4096
bits, textured_case = fc.bits, fc.textured_case


def grid_mesh(nx, ny, origin, ex, ey):
    """An nx x ny grid of quads as (verts, quads [n, 4] counter-clockwise)."""
    o, ex, ey = (np.asarray(a, f32) for a in (origin, ex, ey))
    verts = np.array([o + ex * (i / nx) + ey * (j / ny) for j in range(ny + 1) for i in range(nx + 1)], f32)
    quads = [(j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i) for j in range(ny) for i in range(nx)]
    return verts, np.array(quads, u32)


def fan(polygons):
    """Fan triangulation anchored at each polygon's first vertex, with its face table: (triangles, faces, slices)."""
    tris, faces, slices = [], [], []
    for f, poly in enumerate(polygons):
        n = len(poly)
        for k in range(1, n - 1):
            tris.append((poly[0], poly[k], poly[k + 1]))
            faces.append(f)
            slices.append(fr.TRIANGLE if n == 3 else (fr.UNMAPPABLE if n > 4 else (fr.QUAD_LOWER if k == 1 else fr.QUAD_UPPER)))
    return np.array(tris, u32), np.array(faces, u32), np.array(slices, np.uint8)


@pytest.fixture(scope="module")
def world(crt):
    """-> (scene, maps, bindings): floor of quads (geom 0), wall of triangles (1), a pentagon beside a quad (2), the floor
    mirrored with its winding swapped back (3, bound swapped), one small quad mesh instanced twice (4, 5: the key is the
    instance's id), a sphere (6, bound to nothing)."""
    b = crt.SceneBuilder()
    maps, bindings = [], {}
    fv, fq = grid_mesh(4, 3, (-2, 0, -2), (4, 0, 0), (0, 0, 4))
    ft_, ff, fs = fan(fq.tolist())
    g = b.attach_triangles(fv, ft_)
    maps.append((ff, fs)); bindings[g] = (0, False)
    wv, wq = grid_mesh(3, 2, (-2, 0, -2), (4, 0, 0), (0, 3, 0))
    wt = np.concatenate([[(q[0], q[1], q[2]), (q[0], q[2], q[3])] for q in wq.tolist()]).astype(u32)
    g = b.attach_triangles(wv, wt)
    maps.append((np.arange(len(wt), dtype=u32), np.zeros(len(wt), np.uint8))); bindings[g] = (1, False)
    pv = np.array([(2, 0, -2), (3, 0, -2), (3.5, 1, -2), (2.5, 2, -2), (2, 1, -2), (2, 2.2, -2), (3.5, 2.2, -2), (3.5, 3, -2), (2, 3, -2)], f32)
    pt, pf, ps = fan([[0, 1, 2, 3, 4], [5, 6, 7, 8]])
    g = b.attach_triangles(pv, pt)
    maps.append((pf, ps)); bindings[g] = (2, False)
    mv = fv * np.array([1, 1, -1], f32) + np.array([0, 2.5, 0], f32)  # mirrored in z, lifted: a ceiling
    g = b.attach_triangles(mv, ft_[:, [0, 2, 1]])  # bake_indices' swap for det < 0
    bindings[g] = (0, True)
    sb = crt.SceneBuilder()
    sv, sq = grid_mesh(2, 2, (-0.4, -0.4, 0), (0.8, 0, 0), (0, 0.8, 0))
    st, sf, ss = fan(sq.tolist())
    sb.attach_triangles(sv, st)
    inner = sb.commit()
    maps.append((sf, ss))
    for t in ((-1.0, 1.0, 0.5), (1.0, 1.2, 0.0)):
        g = b.attach_instance(inner, crt.affine(t=t))
        bindings[g] = (3, False)
    b.attach_sphere((0.0, 0.6, -0.5), 0.5)
    return b.commit(), maps, bindings


def rays(rng, n):
    o = rng.normal(size=(n, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * 6.0 + (0, 1.2, 0)).astype(f32)
    target = rng.uniform((-2.6, -0.4, -2.6), (2.6, 3.2, 2.6), size=(n, 3)).astype(f32)
    d = target - o
    out = np.zeros((n, 8), f32)
    out[:, 0:3], out[:, 3:6] = o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    out[:, 7] = np.array([0xFFFFFFFF], u32).view(f32)[0]
    return out


def test_resolve_of_traced_hits_matches_the_restatement(crt, world):
    import torch
    scene, maps, bindings = world
    rng = np.random.default_rng(41)
    ft = fc.aggregate(crt, [fc.texture(rng)], maps, bindings)
    d_hits = scene.intersect_n(crt.rays_to_device(rays(rng, N)), 0.001, float("inf"))
    got = ft.resolve(d_hits).cpu().numpy().view(fc.COORD)
    torch.cuda.synchronize()
    h = crt.hits_to_host(d_hits)
    face, fu, fv = fr.world_resolve(maps, bindings, h["geom_id"], h["prim_id"], h["u"], h["v"])
    assert np.array_equal(got["face_id"], face) and not got["_pad"].any()
    assert np.array_equal(bits(got["u"]), bits(fu)) and np.array_equal(bits(got["v"]), bits(fv))
    # the rays reach every geometry, misses included; every slice, the swapped binding and both instances resolve
    gid = h["geom_id"]
    assert (gid == fc.MISS).sum() > 100 and set(gid[gid != fc.MISS].tolist()) == set(range(7))
    for g, (m, _) in bindings.items():
        sel = gid == g
        assert set(maps[m][1][h["prim_id"][sel]].tolist()) == set(maps[m][1].tolist()), g
    assert (face[gid == 6] == fr.NO_FACE).all() and (face[gid == 3] != fr.NO_FACE).all()
    unmappable = (gid == 2) & (maps[2][1][np.minimum(h["prim_id"], len(maps[2][1]) - 1)] == fr.UNMAPPABLE)
    assert unmappable.sum() > 10 and (face[unmappable] == fr.NO_FACE).all()


def test_resolve_of_edge_case_hits_matches_the_restatement(crt):
    rng = np.random.default_rng(42)
    maps = fc.face_maps(rng, len(fc.SIZES))
    ft = fc.aggregate(crt, [fc.texture(rng)], maps, fc.BINDINGS)
    h = fc.hits(rng, N, maps)
    got = ft.resolve(crt.textures.to_device(h)).cpu().numpy().view(fc.COORD)
    face, fu, fv = fr.world_resolve(maps, fc.BINDINGS, h["geom_id"], h["prim_id"], h["u"], h["v"])
    assert np.array_equal(got["face_id"], face)
    assert np.array_equal(bits(got["u"]), bits(fu)) and np.array_equal(bits(got["v"]), bits(fv))
    assert 0.3 < (face != fr.NO_FACE).mean() < 0.8


def test_texture_eval_matches_the_restatement(crt):
    rng = np.random.default_rng(43)
    sizes, texels = fc.texture(rng)
    other = fc.texture(rng, [(2, 2), (1, 1)])
    ft = fc.aggregate(crt, [other + ((0.1, 0.2, 0.3),), (sizes, texels, (0.5, 0.25, 0.75))])
    q = fc.eval_queries(rng, N, sizes)
    got = ft.eval(1, crt.textures.to_device(q)).cpu().numpy()
    want = fr.texture_eval(sizes, texels, (0.5, 0.25, 0.75), q["face_id"], q["u"], q["v"])
    assert np.array_equal(bits(got), bits(want))
    assert np.isnan(q["u"]).sum() > 50 and (q["face_id"] >= len(sizes)).sum() > 100
    q0 = fc.eval_queries(rng, 1001, other[0])
    got0 = ft.eval(0, crt.textures.to_device(q0)).cpu().numpy()
    assert np.array_equal(bits(got0), bits(fr.texture_eval(other[0], other[1], (0.1, 0.2, 0.3), q0["face_id"], q0["u"], q0["v"])))
    with pytest.raises(crt.CrtError, match="texture 2 of 2"):
        ft.eval(2, crt.textures.to_device(q0))


@pytest.mark.parametrize("cls", sc.CLASSES)
def test_textured_material_calls_match_the_untextured_ones_on_the_substituted_table(crt, cls):
    ft, mats, q, coords, table, q_sub, textured = textured_case(crt, cls, N_SHADE, 3000 + sc.CLASSES.index(cls))
    as_records = lambda t: [crt.CrtMaterial.from_buffer_copy(m.tobytes()) for m in t]
    faced = crt.textures.FacedMaterials(as_records(mats), ft)
    plain, substituted = crt.shading.DeviceMaterials(as_records(mats)), crt.shading.DeviceMaterials(as_records(table))
    d_q, d_sub, d_c = crt.shading.to_device(q), crt.shading.to_device(q_sub), crt.textures.to_device(coords)
    oracle = sc.oracle_drivers()
    for name, dtype in (("scatter_importance", sc.SCATTER_SAMPLE), ("eval", sc.BSDF_EVAL)):
        got = getattr(faced, name)(d_q, d_c).cpu().numpy().view(dtype)
        want = getattr(substituted, name)(d_sub).cpu().numpy().view(dtype)
        bad = sc.mismatches(got, want)
        assert len(bad) == 0, (cls, name, len(bad), got[bad[:2]], want[bad[:2]])
        # ... which is also what the oracle's function answers on that table
        truth = getattr(oracle, "scatter" if name == "scatter_importance" else "eval")(table, q_sub)
        assert len(sc.mismatches(got, truth)) == 0
        # NO_FACE and untextured materials: the untextured call on the original table
        base = getattr(plain, name)(d_q).cpu().numpy().view(dtype)
        assert len(sc.mismatches(got[~textured], base[~textured])) == 0
        if cls != "emissive":
            assert len(sc.mismatches(got[textured], base[textured])) > 0.25 * got["some"][textured].sum()
    # emission keeps the authored colour: the wrapper's emitted_directional is the untextured call
    e = faced.emitted_directional(d_q).cpu().numpy()
    assert np.array_equal(bits(e), bits(plain.emitted_directional(d_q).cpu().numpy()))
