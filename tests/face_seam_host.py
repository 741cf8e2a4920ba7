"""A host integrator that textures from outside (test infrastructure): seam_integrator.SeamHost — the oracle's scalar
trace_path with every seam call handed to Python — that remembers the last `intersect` result (the hook receives geom_id,
prim_id, u, v), checks that the next `scatter` / `eval` is about that hit (rec.t), resolves the hit into a face
coordinate and shades with the texel in the place of base_color. Two texturing backends:
  RefFaces     tests/face_ref.py on the description's own tables, the substituted material run through the seam_cases
               drivers (the oracle's untextured functions): the truth, no GPU, nothing of the library on the textured path
  DeviceFaces  crt_face_resolve_n and crt_material_scatter_faces_n / _eval_faces_n (textures.FaceTextures, FacedMaterials)
Also the procedural loader the scene's tests use in the place of a .ptx decoder."""
import os

import numpy as np

import face_cases as fc
import face_ref as fr
import seam_cases as sc
import seam_integrator as si

f32, u32 = np.float32, np.uint32
CASES = ("quad_lower", "quad_upper", "triangle", "swapped", "instanced", "unmappable_authored", "sphere_authored")


def procedural_loader(crt, n_faces=None):
    """loader(path) -> FaceTexture: faces of 1x1 up to 8x4 texels, colours seeded by the file name; n_faces: {basename:
    count} (default 8)."""
    def load(path):
        name = os.path.basename(path)
        n = (n_faces or {}).get(name, 8)
        rng = np.random.default_rng(sum(name.encode()))
        sizes = [[(1, 1), (2, 2), (4, 4), (8, 4), (4, 8), (2, 1)][k % 6] for k in range(n)]
        texels = rng.uniform(0.05, 0.95, size=(sum(w * h for w, h in sizes), 3)).astype(f32)
        return crt.textures.FaceTexture(sizes, texels)
    return load


SCENE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "face_textured.usda")
SCENE_FACES = {"ground.ptx": 6, "tile.ptx": 2}


def load_scene(crt, width=None, height=None, static_dir=None):
    """scenes/face_textured.usda with the procedural loader. static_dir: a directory to write the scene's second case
    into — the moving placement removed, so nothing moves and no ray carries a time — and load that instead."""
    import re
    import warnings
    path = SCENE
    if static_dir is not None:
        text = open(SCENE).read()
        cut = re.sub(r'    def Mesh "TileMoving".*?\n    }\n\n', "", text, flags=re.S)
        assert cut != text and "crust:motion" not in cut
        path = os.path.join(str(static_dir), "face_textured_static.usda")
        with open(path, "w") as f:
            f.write(cut)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the ceiling strip has two faces under a six-face texture: the warning is tested elsewhere
        desc = crt.usda.load(path, width, height, face_textures=procedural_loader(crt, SCENE_FACES))
    assert any("l2w_end" in g for g in desc.geoms) == (static_dir is None)
    return desc


def truth_host(desc, o):
    """The truth: the oracle's traversal and untextured functions, face_ref choosing the base colour."""
    shade = si.DriversShade(sc.oracle_drivers(), o)
    return FaceSeamHost(si.OracleKernel(o.scene), shade, RefFaces(desc, shade), desc)


class RefFaces:
    def __init__(self, desc, shade):
        self.desc, self.shade = desc, shade
        self.maps = desc.face_maps
        self.bindings = {gid: (g["face_map"], g["face_swapped"]) for gid, g in enumerate(desc.geoms) if "face_map" in g}

    def resolve(self, hit):
        face, fu, fv = fr.world_resolve(self.maps, self.bindings, [hit["geom_id"]], [hit["prim_id"]], [hit["u"]], [hit["v"]])
        return int(face[0]), fu[0], fv[0]

    def _table(self, q, coord):
        m = self.shade.mats[int(q["material"][0]):int(q["material"][0]) + 1].copy()
        tex = self.desc.geoms[int(q["material"][0])]["material"].get("_face_texture")
        if tex is not None and coord[0] != fr.NO_FACE:
            t = self.desc.face_textures[tex]
            sizes = list(zip(t.faces["width"].tolist(), t.faces["height"].tolist()))
            m["base_color"][0] = fr.texture_eval(sizes, t.texels, t.fallback, [coord[0]], [coord[1]], [coord[2]])[0]
        q = q.copy()
        q["material"] = 0
        return m, q

    def scatter(self, q, coord):
        return self.shade.d.scatter(*self._table(q, coord))

    def eval(self, q, coord):
        return self.shade.d.eval(*self._table(q, coord))


class DeviceFaces:
    def __init__(self, crt, ft, materials):
        self.crt, self.ft = crt, ft
        self.faced = crt.textures.FacedMaterials(materials, ft)

    def resolve(self, hit):
        h = np.zeros(1, fc.HIT)
        for k in ("t", "u", "v", "geom_id", "prim_id"):
            h[k] = hit[k]
        self.d_coord = self.ft.resolve(self.crt.textures.to_device(h))
        c = self.d_coord.cpu().numpy().view(fc.COORD)[0]
        return int(c["face_id"]), c["u"], c["v"]

    def scatter(self, q, coord):
        return self.faced.scatter_importance(self.crt.shading.to_device(q), self.d_coord).cpu().numpy().view(sc.SCATTER_SAMPLE)

    def eval(self, q, coord):
        return self.faced.eval(self.crt.shading.to_device(q), self.d_coord).cpu().numpy().view(sc.BSDF_EVAL)


class _TexturedShade:
    """The shade backend SeamHost calls, with scatter / eval routed through the faces backend at the host's coordinate."""

    def __init__(self, host, shade):
        self.host, self.shade = host, shade

    def scatter(self, q):
        return self.host.faces.scatter(q, self.host.coordinate(q, "scatter"))

    def eval(self, q):
        return self.host.faces.eval(q, self.host.coordinate(q, "eval"))

    def __getattr__(self, name):  # emitted and the lights: untextured, as upstream
        return getattr(self.shade, name)


class FaceSeamHost(si.SeamHost):
    def __init__(self, kernel, shade, faces, desc):
        super().__init__(kernel, _TexturedShade(self, shade))
        self.faces, self.desc, self.last, self.scattered_from, self.errors = faces, desc, None, None, []
        self.seen = {(c, m): 0 for c in CASES for m in ("scatter", "eval")}

    def intersect(self, _ctx, ray, t_min, t_max, out):
        rc = super().intersect(_ctx, ray, t_min, t_max, out)
        o = out.contents
        self.last = dict(t=o.t, u=o.u, v=o.v, geom_id=o.geom_id, prim_id=o.prim_id) if rc == 1 else None
        return rc

    def coordinate(self, q, method):
        try:
            return self._coordinate(q, method)
        except Exception as e:  # noqa: BLE001 — kept for the test: ctypes prints and drops what a callback raises
            self.errors.append(e)
            raise

    def _coordinate(self, q, method):
        """The face coordinate of the hit this call shades; tallies which of the seven cases it is."""
        # the hit being shaded is the last one traced — or, for the eval of bounce_emission_weight (tracer.rs:930-953: the
        # PREVIOUS vertex's material, after the bounce ray reached an emitter), the one the last scatter left from. The
        # reference carries face_id / face_uv in that vertex's HitRecord; this host carries the hit with the vertex too, under
        # the vertex's point rec.p as the scatter call stated it: an eval at that very point is about that vertex, every
        # other call is about the last hit traced and must state its t.
        p = q["p"][0].tobytes()
        if method == "eval" and self.scattered_from is not None and self.scattered_from[0] == p:
            hit = self.scattered_from[1]
        else:
            hit = self.last
        assert hit is not None and f32(hit["t"]) == q["t"][0] and int(q["material"][0]) == hit["geom_id"], \
            (method, hit, self.last, q["t"], q["material"])
        if method == "scatter":
            self.scattered_from = (p, hit)
        coord = self.faces.resolve(hit)
        g = self.desc.geoms[hit["geom_id"]]
        if "_face_texture" in g["material"]:
            if "face_map" not in g:
                case = "sphere_authored" if g["kind"] == "sphere" else None
            else:
                sl = int(self.desc.face_maps[g["face_map"]][1][hit["prim_id"]])
                case = ("unmappable_authored" if sl == fr.UNMAPPABLE else "swapped" if g["face_swapped"] else
                        "instanced" if g["kind"] == "instance" else ("triangle", "quad_lower", "quad_upper")[sl])
                assert (coord[0] == fr.NO_FACE) == (sl == fr.UNMAPPABLE)
            if case is not None:
                self.seen[(case, method)] += 1
        return coord
