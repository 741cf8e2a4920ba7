"""Per-face textures without a GPU (include/crt_face_textures.h). Four layers, each compared bit for bit:
  1. tests/face_ref.py — the numpy restatement of FaceMap::resolve and PtexTexture::eval — against the reference's own unit
     tests (rt_world.rs:311-368) and hand-derived answers;
  2. the device source of kernels/faces.hip.h compiled for the host (tests/host_shade/faces_host.cpp) against face_ref on
     100 000 random queries each;
  3. the textured scatter / eval of the device source (MatFace, kernels/shade.hip.h) against the oracle's untextured
     functions run on a per-query material table whose base_color is face_ref's texel;
  4. the object: every refusal of crt_face_textures_new with its reason, the image, the symbol list and the header.
The GPU run of 2 and 3 is tests/test_gpu_face_textures.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import face_cases as fc
import face_ref as fr
import seam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
N_QUERIES = 100000
N_SHADE = 20000  # per lobe class


bits, textured_case = fc.bits, fc.textured_case


# ---- 1. face_ref against the reference's unit tests and hand-derived answers -------------------------------------------
QUAD = ([7, 7], [fr.QUAD_LOWER, fr.QUAD_UPPER])


def resolve1(m, prim, u, v, swapped):
    face, fu, fv = fr.map_resolve(m[0], m[1], [prim], [u], [v], swapped)
    return None if face[0] == fr.NO_FACE else (int(face[0]), float(fu[0]), float(fv[0]))


def test_ref_quad_corners_map_to_the_unit_square():
    assert resolve1(QUAD, 0, 0.0, 0.0, False) == (7, 0.0, 0.0)
    assert resolve1(QUAD, 0, 1.0, 0.0, False) == (7, 1.0, 0.0)
    assert resolve1(QUAD, 0, 0.0, 1.0, False) == (7, 1.0, 1.0)
    assert resolve1(QUAD, 1, 0.0, 0.0, False) == (7, 0.0, 0.0)
    assert resolve1(QUAD, 1, 1.0, 0.0, False) == (7, 1.0, 1.0)
    assert resolve1(QUAD, 1, 0.0, 1.0, False) == (7, 0.0, 1.0)


def test_ref_fan_halves_agree_on_the_shared_diagonal():
    assert resolve1(QUAD, 0, 0.0, 0.5, False) == (7, 0.5, 0.5)
    assert resolve1(QUAD, 1, 0.5, 0.0, False) == (7, 0.5, 0.5)


def test_ref_mirrored_placement_unswaps_barycentrics():
    assert resolve1(QUAD, 0, 1.0, 0.0, True) == (7, 1.0, 1.0)


def test_ref_ngon_slices_have_no_face():
    assert resolve1(([3], [fr.UNMAPPABLE]), 0, 0.25, 0.25, False) is None


def test_ref_out_of_range_prim_id_declines():
    assert resolve1(QUAD, 99, 0.0, 0.0, False) is None


def test_ref_world_lookup_declines_for_misses_and_unbound_geometries():
    face, fu, fv = fr.world_resolve([QUAD], {2: (0, False)}, [2, 1, 0xFFFFFFFF, 2], [0, 0, 0, 1], [0.25] * 4, [0.5] * 4)
    assert face.tolist() == [7, fr.NO_FACE, fr.NO_FACE, 7]
    assert (fu.tolist(), fv.tolist()) == ([0.75, 0.0, 0.0, 0.25], [0.5, 0.0, 0.0, 0.75])


def test_ref_eval_hand_derived_answers():
    sizes = [(4, 2), (1, 1), (0, 3), (2, 2)]
    texels = np.arange(3 * (8 + 1 + 0 + 4), dtype=f32).reshape(-1, 3) / f32(64)
    fallback = (0.5, 0.25, 0.125)

    def ev(face, u, v):
        return fr.texture_eval(sizes, texels, fallback, [face], [u], [v])[0]
    # a texel centre ((i + 0.5) / w, (j + 0.5) / h) returns that texel exactly
    for j in range(2):
        for i in range(4):
            assert np.array_equal(bits(ev(0, (i + 0.5) / 4, (j + 0.5) / 2)), bits(texels[j * 4 + i])), (i, j)
    # u = 0 and u = 1 return the border texel (the neighbour is the same texel: clamped)
    assert np.array_equal(ev(0, 0.0, 0.25), texels[0]) and np.array_equal(ev(0, 1.0, 0.25), texels[3])
    assert np.array_equal(ev(0, 0.0, 1.0), texels[4]) and np.array_equal(ev(0, 1.0, 1.0), texels[7])
    # halfway between two texel centres: the project's lerp, a * (1 - s) + b * s, at s = 0.5
    want = (texels[1] * f32(0.5) + texels[2] * f32(0.5)).astype(f32)
    assert np.array_equal(bits(ev(0, 0.5, 0.25)), bits(want))
    # a 1x1 face answers its texel everywhere
    for u, v in ((0.0, 0.0), (1.0, 1.0), (0.3, 0.9)):
        assert np.array_equal(ev(1, u, v), texels[8])
    # a NaN or infinite coordinate reads as 0
    for bad in (np.nan, np.inf, -np.inf):
        assert np.array_equal(ev(0, bad, 0.25), ev(0, 0.0, 0.25)) and np.array_equal(ev(0, 0.125, bad), ev(0, 0.125, 0.0))
    # outside [0, 1] clamps
    assert np.array_equal(ev(3, -2.0, 7.0), ev(3, 0.0, 1.0))
    # a face id past the table and a 0-wide face give the fallback
    for face in (4, 1000, fr.NO_FACE, 2):
        assert np.array_equal(ev(face, 0.5, 0.5), np.asarray(fallback, f32))


# ---- 2. the device source on the host ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("faces_host") / "libfaces_host.so"
    k = os.path.join(ROOT, "crust-render_amd", "csrc", "kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + k, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host_shade", "faces_host.cpp"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(str(out))
    for name in ("host_face_resolve_n", "host_face_eval_n", "host_face_scatter_n", "host_face_mat_eval_n"):
        getattr(L, name).restype = None
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_device_resolve_matches_the_restatement(crt, host):
    rng = np.random.default_rng(31)
    maps = fc.face_maps(rng, len(fc.SIZES))
    ft = fc.aggregate(crt, [fc.texture(rng)], maps, fc.BINDINGS)
    image = ft.image_bytes()
    h = fc.hits(rng, N_QUERIES, maps)
    got = np.zeros(N_QUERIES, fc.COORD)
    host.host_face_resolve_n(_p(image), _p(h), C.c_size_t(N_QUERIES), _p(got))
    face, fu, fv = fr.world_resolve(maps, fc.BINDINGS, h["geom_id"], h["prim_id"], h["u"], h["v"])
    assert np.array_equal(got["face_id"], face)
    assert np.array_equal(bits(got["u"]), bits(fu)) and np.array_equal(bits(got["v"]), bits(fv))
    # the cases reach what they are meant to: all four slices in both swap states, declines of every kind
    some = face != fr.NO_FACE
    assert 0.3 < some.mean() < 0.8 and (h["geom_id"] == fc.MISS).sum() > 1000
    for g, (m, _) in fc.BINDINGS.items():
        sel = (h["geom_id"] == g) & (h["prim_id"] < len(maps[m][0]))
        seen = set(maps[m][1][h["prim_id"][sel]].tolist())
        assert seen == set(maps[m][1].tolist()), (g, seen)
        assert ((h["geom_id"] == g) & (h["prim_id"] >= len(maps[m][0]))).sum() > 0
    assert (fu[some] == 1.0).sum() > 100 and (fu[some] == 0.0).sum() > 100


def test_device_eval_matches_the_restatement(crt, host):
    rng = np.random.default_rng(32)
    sizes, texels = fc.texture(rng)
    other = fc.texture(rng, [(2, 2), (1, 1)])
    ft = fc.aggregate(crt, [other + ((0.1, 0.2, 0.3),), (sizes, texels, (0.5, 0.25, 0.75))])
    image = ft.image_bytes()
    q = fc.eval_queries(rng, N_QUERIES, sizes)
    got = np.zeros((N_QUERIES, 3), f32)
    host.host_face_eval_n(_p(image), C.c_uint32(1), _p(q), C.c_size_t(N_QUERIES), _p(got))
    want = fr.texture_eval(sizes, texels, (0.5, 0.25, 0.75), q["face_id"], q["u"], q["v"])
    assert np.array_equal(bits(got), bits(want))
    fallback = (want == np.asarray((0.5, 0.25, 0.75), f32)).all(axis=1)
    assert 0.1 < fallback.mean() < 0.4 and np.isnan(q["u"]).sum() > 500 and np.isinf(q["v"]).sum() > 500
    assert set(q["face_id"][q["face_id"] < len(sizes)].tolist()) == set(range(len(sizes)))
    # the second texture of the image does not leak into the first
    q0 = fc.eval_queries(rng, 4096, other[0])
    got0 = np.zeros((4096, 3), f32)
    host.host_face_eval_n(_p(image), C.c_uint32(0), _p(q0), C.c_size_t(4096), _p(got0))
    assert np.array_equal(bits(got0), bits(fr.texture_eval(other[0], other[1], (0.1, 0.2, 0.3), q0["face_id"], q0["u"], q0["v"])))


# ---- 3. textured scatter / eval against the untextured functions on the substituted table --------------------------------
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_textured_material_methods_match_the_untextured_ones_on_the_substituted_table(crt, host, cls):
    ft, mats, q, coords, table, q_sub, textured = textured_case(crt, cls, N_SHADE, 2000 + sc.CLASSES.index(cls))
    oracle = sc.oracle_drivers()
    image = ft.image_bytes()
    assert 0.4 < textured.mean() < 0.7
    for name, fn, dtype in (("scatter", "host_face_scatter_n", sc.SCATTER_SAMPLE), ("eval", "host_face_mat_eval_n", sc.BSDF_EVAL)):
        got = np.zeros(N_SHADE, dtype)
        getattr(host, fn)(_p(image), _p(mats), C.c_size_t(len(mats)), _p(q), _p(coords), C.c_size_t(N_SHADE), _p(got))
        want = getattr(oracle, name)(table, q_sub)
        bad = sc.mismatches(got, want)
        assert len(bad) == 0, (cls, name, len(bad), got[bad[:2]], want[bad[:2]])
        # a query without a texture or without a face is the untextured call on the original table
        plain = getattr(oracle, name)(mats, q)
        assert len(sc.mismatches(got[~textured], plain[~textured])) == 0
        # and the texture does change answers where it applies (not all of them: an eval towards the far side of an
        # opaque surface is zero whatever the colour, and so is a scatter that returns None)
        if cls != "emissive":
            assert len(sc.mismatches(got[textured], plain[textured])) > 0.25 * got["some"][textured].sum()


# ---- 4. the object, no device ---------------------------------------------------------------------------------------------
def test_symbol_list_header_and_library_agree(crt):
    text = open(os.path.join(ROOT, "include", "crt_face_textures.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crt_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(crt.ABI_SYMBOLS_FACE_TEXTURES), set(names) ^ set(crt.ABI_SYMBOLS_FACE_TEXTURES)
    for name in names:
        assert hasattr(crt.lib(), name), name
    # beside crt.h, not in it: the three older lists and crt.h's own stay as they are
    assert not set(names) & set(crt.ABI_SYMBOLS + crt.ABI_SYMBOLS_RENDER_VOLUMES + crt.ABI_SYMBOLS_SCENE_IMAGE + crt.ABI_SYMBOLS_GUIDING)
    assert "face_textures" not in open(os.path.join(ROOT, "include", "crt.h")).read().replace("crt_face_textures.h", "")


def test_struct_sizes_match_the_header(crt, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "crt_face_textures.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(CrtFaceRect), sizeof(CrtFaceTexture), sizeof(CrtFaceMap), sizeof(CrtFaceBinding), sizeof(CrtFaceCoord), "
                   "sizeof(CrtFaceTexturesHeader)); return 0; }\n")
    exe = str(tmp_path / "sizes")
    res = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    T = crt.textures
    want = [T.FACE_RECT.itemsize, C.sizeof(T._CrtFaceTexture), C.sizeof(T._CrtFaceMap), T.BINDING.itemsize, T.COORD.itemsize,
            T.IMAGE_HEADER.itemsize]
    assert [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()] == want


def test_image_round_trips_the_inputs(crt):
    rng = np.random.default_rng(33)
    maps = fc.face_maps(rng, len(fc.SIZES))
    tex = [fc.texture(rng) + ((0.1, 0.2, 0.3),), fc.texture(rng, [(2, 3), (0, 0), (1, 1)])]
    ft = fc.aggregate(crt, tex, maps, fc.BINDINGS, [0, None, 1, 1])
    im = ft.image()
    hd = im["header"]
    assert hd["bytes"] == len(ft.image_bytes()) and hd["n_textures"] == 2 and hd["n_maps"] == 3 and hd["n_materials"] == 4
    assert hd["n_geoms"] == max(fc.BINDINGS) + 1
    assert im["material_texture"].tolist() == [0, 0xFFFFFFFF, 1, 1]
    assert np.array_equal(im["textures"]["fallback"], np.array([(0.1, 0.2, 0.3), (0.5, 0.5, 0.5)], f32))
    first_texel = 0
    for t, (sizes, texels, *_) in enumerate(tex):
        rec = im["textures"][t]
        faces = im["faces"][rec["first_face"]:rec["first_face"] + rec["n_faces"]]
        assert list(zip(faces["width"].tolist(), faces["height"].tolist())) == [tuple(s) for s in sizes]
        area = np.array([w * h for w, h in sizes])
        assert np.array_equal(faces["texel"], first_texel + np.concatenate([[0], np.cumsum(area)[:-1]]))
        got = im["texels"][first_texel:first_texel + len(texels)]
        assert np.array_equal(bits(got[:, :3]), bits(texels)) and not got[:, 3].any()
        first_texel += len(texels)
    for m, (faces, slices) in enumerate(maps):
        rec = im["maps"][m]
        assert rec["n_prims"] == len(faces)
        assert np.array_equal(im["map_faces"][rec["first_prim"]:rec["first_prim"] + rec["n_prims"]], faces)
        assert np.array_equal(im["map_slices"][rec["first_prim"]:rec["first_prim"] + rec["n_prims"]], slices)
    for g in range(int(hd["n_geoms"])):
        want = 0xFFFFFFFF if g not in fc.BINDINGS else fc.BINDINGS[g][0] | (0x80000000 if fc.BINDINGS[g][1] else 0)
        assert im["geoms"][g] == want, g
    ft.close()
    # an empty aggregate is legal and resolves nothing
    empty = crt.textures.FaceTextures([])
    assert empty.image()["header"]["n_textures"] == 0
    empty.close()


def refused(crt, *args, **kw):
    with pytest.raises(crt.CrtError) as e:
        fc.aggregate(crt, *args, **kw)
    return str(e.value)


def test_every_refusal_names_its_reason(crt):
    rng = np.random.default_rng(34)
    T = crt.textures
    sizes, texels = fc.texture(rng, [(2, 2), (4, 1)])
    good_map = ([0, 0], [fr.QUAD_LOWER, fr.QUAD_UPPER])
    # a dangling index
    assert "binding 0 names map 1 of 1" in refused(crt, [(sizes, texels)], [good_map], {3: (1, False)})
    assert "material 1 names texture 1 of 1" in refused(crt, [(sizes, texels)], material_texture=[0, 1])
    assert "names geometry %d" % T.MAX_GEOMS in refused(crt, [(sizes, texels)], [good_map], {T.MAX_GEOMS: (0, False)})
    # a face whose texels run past the texel array
    assert "face 1 of texture 0 reads texels 4 .. 8 of 7" in refused(crt, [(sizes, texels[:7])])
    rects = np.array([(0xFFFFFFFF, 2, 2)], T.FACE_RECT)  # an offset that would wrap in 32 bits
    with pytest.raises(crt.CrtError, match="reads texels 4294967295 .. 4294967299 of 8"):
        T.FaceTextures([T.FaceTexture(rects, texels)])
    # a slice value above 3
    assert "primitive 1 of map 0 has the unknown slice 4" in refused(crt, [(sizes, texels)], [([0, 0], [1, 4])])
    # a non-finite texel or fallback
    for bad in (np.nan, np.inf, -np.inf):
        broken = texels.copy()
        broken[5, 1] = bad
        assert "texel 5 of texture 0 has a channel that is not finite" in refused(crt, [(sizes, broken)])
        assert "texture 0 has a fallback colour that is not finite" in refused(crt, [(sizes, texels, (0.5, bad, 0.5))])
    # sizes past the limits: a face above 16384 either way (its texels need not exist for the refusal)
    rects = np.array([(0, T.MAX_RES + 1, 1)], T.FACE_RECT)
    with pytest.raises(crt.CrtError, match="is 16385 x 1 texels"):
        T.FaceTextures([T.FaceTexture(rects, texels)])
    # the limit itself is legal: a 16384-wide face of one row
    wide = T.FaceTextures([T.FaceTexture([(T.MAX_RES, 1)], np.zeros((T.MAX_RES, 3), f32))])
    assert wide.image()["faces"]["width"][0] == T.MAX_RES
    wide.close()
    # two bindings of one geometry
    L = crt.lib()
    bind = np.array([(2, 0, 0), (2, 0, 1)], T.BINDING)
    faces, slices = np.array([0, 0], u32), np.array([1, 2], np.uint8)
    cm = T._CrtFaceMap(faces.ctypes.data, slices.ctypes.data, 2)
    assert not L.crt_face_textures_new(None, 0, C.byref(cm), 1, _p(bind), 2, None, 0)
    assert "binding 1 names geometry 2, which is bound already" in L.crt_last_error().decode()
    # a NULL array with a non-zero count
    for args in ((None, 1, None, 0, None, 0, None, 0), (None, 0, None, 1, None, 0, None, 0), (None, 0, None, 0, None, 1, None, 0),
                 (None, 0, None, 0, None, 0, None, 1)):
        assert not L.crt_face_textures_new(*args)
        assert "a NULL array with a non-zero count" in L.crt_last_error().decode()
    ct = T._CrtFaceTexture(None, 3, None, 0, (C.c_float * 3)(0.5, 0.5, 0.5))
    assert not L.crt_face_textures_new(C.byref(ct), 1, None, 0, None, 0, None, 0)
    assert "texture 0 has a NULL array with a non-zero count" in L.crt_last_error().decode()
    cm = T._CrtFaceMap(None, None, 5)
    assert not L.crt_face_textures_new(None, 0, C.byref(cm), 1, None, 0, None, 0)
    assert "map 0 has a NULL array with a non-zero count" in L.crt_last_error().decode()


def test_a_device_image_of_4_gib_is_refused_before_it_is_built(crt):
    """2^28 texels are 4 GiB of 16-byte device texels: refused on the count, with no allocation and no read of the texels
    (the array handed in here is far shorter than the count claims, which a refusal on the count never notices)."""
    T, L = crt.textures, crt.lib()
    few = np.zeros((4, 3), f32)
    ct = T._CrtFaceTexture(None, 0, few.ctypes.data, 1 << 28, (C.c_float * 3)(0.5, 0.5, 0.5))
    assert not L.crt_face_textures_new(C.byref(ct), 1, None, 0, None, 0, None, 0)
    assert "the device image would reach 4 GiB" in L.crt_last_error().decode()


def test_entry_points_check_their_arguments_without_a_device(crt):
    L = crt.lib()
    ft = fc.aggregate(crt, [fc.texture(np.random.default_rng(35), [(1, 1)])])
    p, n = C.c_void_p(), C.c_size_t()
    assert L.crt_face_textures_image(None, C.byref(p), C.byref(n)) == -1 and L.crt_face_textures_image(ft.h, None, C.byref(n)) == -1
    one = C.c_void_p(16)  # never dereferenced: the checks come first
    assert L.crt_face_resolve_n(None, one, 1, one, None) == -1 and L.crt_face_resolve_n(ft.h, None, 1, one, None) == -1
    assert L.crt_face_resolve_n(ft.h, None, 0, None, None) == 0  # nothing to do
    assert L.crt_face_texture_eval_n(ft.h, 1, one, 1, one, None) == -1
    assert "texture 1 of 1" in L.crt_last_error().decode()
    assert L.crt_face_texture_eval_n(ft.h, 0, one, 0, one, None) == 0
    assert L.crt_material_scatter_faces_n(None, one, 1, one, one, 1, one, None) == -1
    assert L.crt_material_scatter_faces_n(ft.h, one, 1, one, None, 1, one, None) == -1
    assert L.crt_material_eval_faces_n(ft.h, None, 1, one, one, 1, one, None) == -1
    assert L.crt_material_eval_faces_n(ft.h, one, 1, one, one, 0, one, None) == 0
    L.crt_face_textures_free(None)  # a no-op
    ft.close()


# ---- sanitizers: a stand-alone program, on the CPU ---------------------------------------------------------------------
def test_builder_refusals_and_edge_queries_are_clean_under_asan_and_ubsan(tmp_path):
    """profiles/host_shade/face_textures_sanitize.cpp: face_textures.cpp's builder and the host-compiled resolve / eval in a
    program of their own (its own main), built with -fsanitize=address,undefined; nothing of it is loaded into Python."""
    exe = tmp_path / "face_textures_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "profiles", "host_shade"),
           "-I" + os.path.join(ROOT, "crust-render_amd", "csrc"),
           os.path.join(ROOT, "profiles", "host_shade", "face_textures_sanitize.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "face_textures_sanitize: 12 refusals, 35100 queries, 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
