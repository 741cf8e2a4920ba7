"""The importer's side of per-face textures, without a GPU: usda.load(..., face_textures=loader) — the PxrDisneyBsdf arm
(usd_import.rs:2745-2806), inputs:surfaceMap through the loader (:2814-2841), the face tables of _triangulate
(:1164-1214, with the reference's own face_table_tests restated), the swap rule of baked and instanced placements
(:1054-1078) and the face-count warning (:1140-1153) — and build_face_textures."""
import os
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = os.path.join(ROOT, "tests", "golden", "face_disney.usda")
f32 = np.float32


class Loader:
    """AssetLoader::load_ptex: remembers what it was asked for; answers a texture of n_faces 1x1 faces, or None for a
    path it is told to decline."""

    def __init__(self, crt, n_faces=1, decline=()):
        self.crt, self.n_faces, self.decline, self.asked = crt, n_faces, decline, []

    def __call__(self, path):
        self.asked.append(path)
        if os.path.basename(path) in self.decline:
            return None
        return self.crt.textures.FaceTexture([(1, 1)] * self.n_faces, np.full((self.n_faces, 3), 0.25, f32))


def by_name(desc):
    return {g["name"]: (gid, g) for gid, g in enumerate(desc.geoms)}


# ---- _triangulate: the reference's face_table_tests -------------------------------------------------------------------------
def test_quad_mesh_face_table_is_parallel_to_triangles(crt):
    tris, faces, slices = crt.usda._triangulate([4, 4, 4], list(range(12)), 12, True)
    assert len(tris) == 6 and faces.tolist() == [0, 0, 1, 1, 2, 2] and slices.tolist() == [1, 2, 1, 2, 1, 2]
    assert tris[2].tolist() == [4, 5, 6] and tris[3].tolist() == [4, 6, 7]


def test_skipped_faces_do_not_shift_later_face_ids(crt):
    tris, faces, _ = crt.usda._triangulate([4, 2, 4], list(range(10)), 10, True)
    assert len(tris) == 4 and faces.tolist() == [0, 0, 2, 2]
    # a triangle dropped for an index past the vertices leaves the rest of its face, and the faces after it, alone
    tris, faces, slices = crt.usda._triangulate([4, 3], [0, 1, 2, 99, 3, 4, 5], 6, True)
    assert tris.tolist() == [[0, 1, 2], [3, 4, 5]] and faces.tolist() == [0, 1] and slices.tolist() == [1, 0]


def test_ngons_and_triangles_get_their_own_slices(crt):
    _, faces, slices = crt.usda._triangulate([3, 5], list(range(8)), 8, True)
    assert slices.tolist() == [0, 3, 3, 3] and faces.tolist() == [0, 1, 1, 1]


def test_face_table_is_not_built_unless_requested(crt):
    tris = crt.usda._triangulate([4], [0, 1, 2, 3], 4)
    assert isinstance(tris, np.ndarray) and tris.tolist() == [[0, 1, 2], [0, 2, 3]]
    T = crt.textures
    assert (T.FAN_TRIANGLE, T.FAN_QUAD_LOWER, T.FAN_QUAD_UPPER, T.FAN_UNMAPPABLE) == (0, 1, 2, 3)


# ---- the loader -------------------------------------------------------------------------------------------------------------
def test_each_resolved_path_is_loaded_once_and_negative_answers_are_cached(crt):
    loader = Loader(crt, decline=("missing.ptx",))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        desc = crt.usda.load(STAGE, 16, 16, face_textures=loader)
    here = os.path.dirname(STAGE)
    # four meshes under two materials name nonexistent.ptx, resolved against the layer's directory: one load; missing.ptx
    # is declined once and not asked for again
    assert sorted(loader.asked) == [os.path.join(here, "missing.ptx"), os.path.join(here, "nonexistent.ptx")]
    assert len(desc.face_textures) == 1
    geoms = by_name(desc)
    for name in ("Quad", "Mirrored", "TwiceA", "TwiceB"):
        assert geoms[name][1]["material"]["_face_texture"] == 0, name
    assert "_face_texture" not in geoms["Plain"][1]["material"] and "face_map" not in geoms["Plain"][1]


def test_without_the_keyword_the_description_is_todays(crt):
    desc = crt.usda.load(STAGE, 16, 16)
    assert not hasattr(desc, "face_textures") and not hasattr(desc, "face_maps")
    for g in desc.geoms:
        assert g["material"] is crt.usda.DEFAULT_MATERIAL  # a Disney material still reads as default grey
        assert "face_map" not in g and "face_swapped" not in g
    # and a stage without any such material is the same description with or without a loader
    path = os.path.join(ROOT, "scenes", "veach_mis.usda")
    loader = Loader(crt)
    a, b = crt.usda.load(path, 32, 18), crt.usda.load(path, 32, 18, face_textures=loader)
    assert loader.asked == [] and b.face_textures == [] and b.face_maps == []

    def same(x, y):
        if isinstance(x, dict):
            return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, np.ndarray):
            return np.array_equal(x, y)
        return x == y
    assert same(a.geoms, b.geoms) and same(a.protos, b.protos) and same(a.lights, b.lights) and same(a.camera, b.camera)
    assert same(a.settings, b.settings)


# ---- face tables and the swap rule --------------------------------------------------------------------------------------------
def test_face_tables_and_the_swap_rule(crt):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        desc = crt.usda.load(STAGE, 16, 16, face_textures=Loader(crt, decline=("missing.ptx",)))
    geoms = by_name(desc)
    # a sole, unmirrored placement: baked, unswapped; a quad
    _, quad = geoms["Quad"]
    assert quad["kind"] == "mesh" and quad["face_swapped"] is False
    faces, slices = desc.face_maps[quad["face_map"]]
    assert faces.tolist() == [0, 0] and slices.tolist() == [1, 2]
    # a sole, mirrored placement: baked with the winding swapped — the same test as the index swap — and bound swapped;
    # a quad, a triangle and a pentagon, index-parallel with the baked triangles
    _, mir = geoms["Mirrored"]
    assert mir["kind"] == "mesh" and mir["face_swapped"] is True
    faces, slices = desc.face_maps[mir["face_map"]]
    assert faces.tolist() == [0, 0, 1, 2, 2, 2] and slices.tolist() == [1, 2, 0, 3, 3, 3]
    assert len(mir["idx"]) == len(faces) and mir["idx"][0].tolist() == [0, 2, 1]
    # two placements of one mesh: instanced, one shared table, unswapped even where the placement mirrors
    (_, a), (_, b) = geoms["TwiceA"], geoms["TwiceB"]
    assert a["kind"] == b["kind"] == "instance" and a["proto"] == b["proto"] and a["face_map"] == b["face_map"]
    assert a["face_swapped"] is False and b["face_swapped"] is False
    assert desc.face_maps[a["face_map"]][0].tolist() == [0, 0, 1, 1]
    assert len(desc.face_maps) == 3


def test_face_count_warning(crt):
    with pytest.warns(UserWarning, match=r"Mesh at /World/Mirrored has 3 faces but its per-face texture has 1") as rec:
        crt.usda.load(STAGE, 16, 16, face_textures=Loader(crt))
    text = [str(w.message) for w in rec]
    assert any("/World/TwiceA has 2 faces" in t or "/World/TwiceB has 2 faces" in t for t in text)
    assert not any("/World/Quad " in t for t in text)  # one face, one face: no warning


# ---- the Disney mapping -------------------------------------------------------------------------------------------------------
def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def test_disney_inputs_map_onto_openpbr(crt):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        desc = crt.usda.load(STAGE, 16, 16, face_textures=Loader(crt, decline=("missing.ptx",)))
    geoms = by_name(desc)
    moss = geoms["TwiceA"][1]["material"]
    # baseColor 0 and 1 are exact; 0.5^2.2 within 2 ulp of float32 pow (a host powf is not reproducible across libms)
    assert moss["base_color"][0] == 0.0 and moss["base_color"][1] == 1.0
    assert ulps(moss["base_color"][2], np.float32(np.float64(0.5) ** 2.2)) <= 2
    want = dict(base_metalness=0.25, specular_roughness=0.75, specular_ior=1.33, specular_roughness_anisotropy=0.125,
                coat_weight=0.5, coat_roughness=0.125, transmission_weight=0.0625, geometry_opacity=0.9375, thin_walled=1)
    for k, v in want.items():  # as float32, the record's precision (fill_material rounds)
        assert f32(moss[k]) == f32(v), k
    assert "fuzz_weight" not in moss  # sheen is not mapped
    # only authored inputs are mapped: Rock authors roughness alone
    rock = geoms["Quad"][1]["material"]
    assert {k for k in rock if not k.startswith("_")} == {"specular_roughness"} and rock["specular_roughness"] == 0.5
    # negative and above-one components: max(0)^2.2; gloss above one clamps; specularTransmission wins over refractionGain
    bare = geoms["Plain"][1]["material"]
    assert bare["base_color"][2] == 0.0 and ulps(bare["base_color"][1], np.float32(np.float64(1.5) ** 2.2)) <= 2
    assert ulps(bare["base_color"][0], np.float32(np.float64(np.float32(0.2)) ** 2.2)) <= 2
    assert bare["coat_roughness"] == 0.0 and bare["transmission_weight"] == 0.375
    # and the record build_world fills from it
    m = crt.usda.fill_material(crt.default_material(), moss)
    assert (m.base_metalness, m.thin_walled, m.coat_roughness) == (0.25, 1, 0.125) and m.fuzz_weight == crt.default_material().fuzz_weight


# ---- the aggregate ------------------------------------------------------------------------------------------------------------
def test_build_face_textures_binds_geometries_and_materials(crt):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        desc = crt.usda.load(STAGE, 16, 16, face_textures=Loader(crt, decline=("missing.ptx",)))
        plain = crt.usda.load(STAGE, 16, 16)
    assert crt.usda.build_face_textures(plain, crt) is None
    ft = crt.usda.build_face_textures(desc, crt)
    im = ft.image()
    geoms = by_name(desc)
    want_geoms = np.full(int(im["header"]["n_geoms"]), 0xFFFFFFFF, np.uint32)
    for name in ("Quad", "Mirrored", "TwiceA", "TwiceB"):
        gid, g = geoms[name]
        want_geoms[gid] = g["face_map"] | (0x80000000 if g["face_swapped"] else 0)
    assert np.array_equal(im["geoms"], want_geoms)
    mt = im["material_texture"]
    assert len(mt) == len(desc.geoms) and mt[geoms["Plain"][0]] == 0xFFFFFFFF and mt[geoms["Mirrored"][0]] == 0
    assert int(im["header"]["n_maps"]) == 3 and int(im["header"]["n_textures"]) == 1
