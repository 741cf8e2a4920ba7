"""Per-face (Ptex-style) colour textures as callable device functions — host mirror of `PtexTexture` as the reference's
renderer decodes it (crates/crust-render/src/main.rs:172-319), `FaceMap` (crates/crust-core/src/rt_world.rs:20-78),
`World::faces` and `base_color_ptex`, over the C ABI's entry points (include/crt_face_textures.h: crt_face_textures_new /
_free / _image, crt_face_resolve_n, crt_face_texture_eval_n, crt_material_scatter_faces_n, crt_material_eval_faces_n).

The host decodes; the library owns a device image; the kernels only ask it for a value. A host integrator that keeps its
own trace_path resolves the hits of Scene.intersect_n into face coordinates (`FaceTextures.resolve`) and shades them
through `FacedMaterials`, whose scatter_importance / eval put the texel in the place of base_color before the lobe pmf is
built (openpbr.rs:1011-1024). Records live in HBM as torch uint8 tensors; numpy structured dtypes name their fields on the
host. There is no CPU fallback: resolve, eval and the material calls launch kernels of libcrt_amd.so. Building the
aggregate and reading its image need no device.
"""
import ctypes as C

import numpy as np

NO_FACE = 0xFFFFFFFF
INVALID_ID = 0xFFFFFFFF
MAX_RES, MAX_GEOMS = 16384, 1 << 24
FAN_TRIANGLE, FAN_QUAD_LOWER, FAN_QUAD_UPPER, FAN_UNMAPPABLE = 0, 1, 2, 3

_f, _u = np.float32, np.uint32
FACE_RECT = np.dtype([("offset", _u), ("width", np.uint16), ("height", np.uint16)])
BINDING = np.dtype([("geom_id", _u), ("map", _u), ("swapped", _u)])
COORD = np.dtype([("face_id", _u), ("u", _f), ("v", _f), ("_pad", _u)])
# the image crt_face_textures_image hands out (include/crt_face_textures.h: CrtFaceTexturesHeader)
IMAGE_HEADER = np.dtype([(n, _u) for n in (
    "magic", "bytes", "n_textures", "n_faces_total", "n_maps", "n_prims_total", "n_geoms", "n_materials", "n_texels_total",
    "off_textures", "off_faces", "off_maps", "off_map_faces", "off_map_slices", "off_geoms", "off_material_texture", "off_texels")])
IMAGE_TEXTURE = np.dtype([("first_face", _u), ("n_faces", _u), ("fallback", _f, 3), ("_pad", _u, 3)])
IMAGE_FACE = np.dtype([("texel", _u), ("width", np.uint16), ("height", np.uint16)])
IMAGE_MAP = np.dtype([("first_prim", _u), ("n_prims", _u), ("_pad", _u, 2)])
assert (FACE_RECT.itemsize, BINDING.itemsize, COORD.itemsize) == (8, 12, 16)
assert (IMAGE_HEADER.itemsize, IMAGE_TEXTURE.itemsize, IMAGE_FACE.itemsize, IMAGE_MAP.itemsize) == (68, 32, 8, 16)


class _CrtFaceTexture(C.Structure):
    _fields_ = [("faces", C.c_void_p), ("n_faces", C.c_size_t), ("texels", C.c_void_p), ("n_texels", C.c_size_t),
                ("fallback", C.c_float * 3)]


class _CrtFaceMap(C.Structure):
    _fields_ = [("faces", C.c_void_p), ("slices", C.c_void_p), ("n_prims", C.c_size_t)]


def _crt():
    import sys
    return sys.modules[__name__.rsplit(".", 1)[0]]


class FaceTexture:
    """One decoded texture. sizes: per face (width, height), its texels packed one face after the other in face order, or
    FACE_RECT records (offset in texels, width, height) for any other packing; texels: float32 [n, 3] linear RGB,
    row-major within a face, v-major; fallback: the colour of a face that does not exist or has no texels."""

    def __init__(self, sizes, texels, fallback=(0.5, 0.5, 0.5)):
        if isinstance(sizes, np.ndarray) and sizes.dtype == FACE_RECT:
            self.faces = np.ascontiguousarray(sizes)
        else:
            wh = np.asarray(sizes, np.int64).reshape(-1, 2)
            self.faces = np.zeros(len(wh), FACE_RECT)
            area = wh[:, 0] * wh[:, 1]
            self.faces["offset"] = np.concatenate([[0], np.cumsum(area)[:-1]]) if len(wh) else []
            self.faces["width"], self.faces["height"] = wh[:, 0], wh[:, 1]
        self.texels = np.ascontiguousarray(np.asarray(texels, _f).reshape(-1, 3))
        self.fallback = np.broadcast_to(np.asarray(fallback, _f), 3).copy()

    @property
    def n_faces(self):
        return len(self.faces)


class FaceMap:
    """FaceMap (rt_world.rs:43-48): per triangle, indexed by prim_id, the source polygon and its FAN_* slice."""

    def __init__(self, faces, slices):
        self.faces = np.ascontiguousarray(np.asarray(faces, _u).reshape(-1))
        self.slices = np.ascontiguousarray(np.asarray(slices, np.uint8).reshape(-1))
        if len(self.faces) != len(self.slices):
            raise ValueError("FaceMap: faces and slices are index-parallel")


def to_device(records, device="cuda:0"):
    """numpy array -> torch uint8 tensor in HBM."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).to(device)


class FaceTextures:
    """The aggregate over crt_face_textures_new: textures [FaceTexture], maps [FaceMap], bindings [(geom_id, map,
    swapped)] (World::set_face_map: the key is the top-level geom_id a hit reports) and material_texture [texture index
    or None per material] (base_color_ptex). Host only until resolve / eval first run. Raises CrtError with the library's
    reason when the aggregate is refused."""

    def __init__(self, textures, maps=(), bindings=(), material_texture=()):
        crt = _crt()
        self.textures, self.maps = list(textures), list(maps)
        self.bindings = np.zeros(len(bindings), BINDING)
        for rec, b in zip(self.bindings, bindings):
            rec["geom_id"], rec["map"], rec["swapped"] = int(b[0]), int(b[1]), 1 if b[2] else 0
        self.material_texture = np.array([INVALID_ID if t is None else int(t) for t in material_texture], np.int64).astype(_u)
        ct = (_CrtFaceTexture * max(len(self.textures), 1))()
        for c, t in zip(ct, self.textures):
            c.faces, c.n_faces = (t.faces.ctypes.data if len(t.faces) else None), len(t.faces)
            c.texels, c.n_texels = (t.texels.ctypes.data if len(t.texels) else None), len(t.texels)
            c.fallback[:] = [float(x) for x in t.fallback]
        cm = (_CrtFaceMap * max(len(self.maps), 1))()
        for c, m in zip(cm, self.maps):
            c.faces, c.slices, c.n_prims = (m.faces.ctypes.data if len(m.faces) else None), (m.slices.ctypes.data if len(m.faces) else None), len(m.faces)
        self.h = crt.lib().crt_face_textures_new(
            C.cast(ct, C.c_void_p) if self.textures else None, len(self.textures), C.cast(cm, C.c_void_p) if self.maps else None, len(self.maps),
            C.c_void_p(self.bindings.ctypes.data) if len(self.bindings) else None, len(self.bindings),
            C.c_void_p(self.material_texture.ctypes.data) if len(self.material_texture) else None, len(self.material_texture))
        if not self.h:
            raise crt.CrtError(-1, "crt_face_textures_new")

    def close(self):
        """Drops the handle now (crt_face_textures_free); the object is unusable afterwards."""
        h, self.h = getattr(self, "h", None), None
        if h:
            _crt().lib().crt_face_textures_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image_bytes(self):
        """The image the kernels read (crt_face_textures_image), as a numpy uint8 copy."""
        crt = _crt()
        p, n = C.c_void_p(), C.c_size_t()
        crt._check(crt.lib().crt_face_textures_image(self.h, C.byref(p), C.byref(n)), "crt_face_textures_image")
        return np.frombuffer(C.string_at(p.value, n.value), np.uint8).copy()

    def image(self):
        """The image's parts as a dict: header, textures (IMAGE_TEXTURE), faces (IMAGE_FACE, texel offsets absolute), maps
        (IMAGE_MAP), map_faces, map_slices, geoms (map | swapped << 31, or INVALID_ID), material_texture, texels [n, 4]."""
        raw = self.image_bytes()
        hd = raw[:IMAGE_HEADER.itemsize].view(IMAGE_HEADER)[0]

        def part(off, count, dtype):
            dtype = np.dtype(dtype)
            return raw[int(hd[off]):int(hd[off]) + int(count) * dtype.itemsize].view(dtype).copy()
        return dict(header=hd, textures=part("off_textures", hd["n_textures"], IMAGE_TEXTURE),
                    faces=part("off_faces", hd["n_faces_total"], IMAGE_FACE), maps=part("off_maps", hd["n_maps"], IMAGE_MAP),
                    map_faces=part("off_map_faces", hd["n_prims_total"], _u), map_slices=part("off_map_slices", hd["n_prims_total"], np.uint8),
                    geoms=part("off_geoms", hd["n_geoms"], _u), material_texture=part("off_material_texture", hd["n_materials"], _u),
                    texels=part("off_texels", 4 * int(hd["n_texels_total"]), _f).reshape(-1, 4))

    def resolve(self, d_hits, stream=None):
        """World::intersect's face lookup (rt_world.rs:207-232): CrtRayHit records as Scene.intersect_n wrote them (uint8
        device tensor) -> COORD records."""
        import torch
        crt = _crt()
        n = d_hits.numel() * d_hits.element_size() // 40
        d_out = torch.empty(max(n * COORD.itemsize, 1), dtype=torch.uint8, device=d_hits.device)
        crt._check(crt.lib().crt_face_resolve_n(self.h, C.c_void_p(d_hits.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                               crt._stream_ptr(stream)), "crt_face_resolve_n")
        return d_out[:n * COORD.itemsize]

    def eval(self, texture, d_coords, stream=None):
        """PtexTexture::eval (main.rs:277-314): COORD records -> float32 device tensor [n, 3]."""
        import torch
        crt = _crt()
        n = d_coords.numel() * d_coords.element_size() // COORD.itemsize
        d_out = torch.empty(max(3 * n, 1), dtype=torch.float32, device=d_coords.device)
        crt._check(crt.lib().crt_face_texture_eval_n(self.h, int(texture), C.c_void_p(d_coords.data_ptr()), n,
                                                    C.c_void_p(d_out.data_ptr()), crt._stream_ptr(stream)), "crt_face_texture_eval_n")
        return d_out[:3 * n].reshape(n, 3)


class FacedMaterials:
    """shading.DeviceMaterials with OpenPBR::shaded's substitution: a material table in HBM beside a FaceTextures whose
    material_texture is indexed like it. scatter_importance / eval take the queries and their COORD records."""

    def __init__(self, materials, face_textures, device="cuda:0"):
        crt = _crt()
        self.table = materials if isinstance(materials, crt.shading.DeviceMaterials) else crt.shading.DeviceMaterials(materials, device)
        self.ft = face_textures

    def _launch(self, fn, d_queries, d_coords, out_bytes, stream):
        import torch
        crt = _crt()
        n = d_queries.numel() * d_queries.element_size() // 80
        if d_coords.numel() * d_coords.element_size() != n * COORD.itemsize:
            raise ValueError(f"{fn}: {n} queries need {n} coordinates")
        d_out = torch.empty(max(n * out_bytes, 1), dtype=torch.uint8, device=d_queries.device)
        rc = getattr(crt.lib(), fn)(self.ft.h, C.c_void_p(self.table.d.data_ptr() if self.table.n else 0), self.table.n,
                                    C.c_void_p(d_queries.data_ptr()), C.c_void_p(d_coords.data_ptr()), n,
                                    C.c_void_p(d_out.data_ptr()), crt._stream_ptr(stream))
        crt._check(rc, fn)
        return d_out[:n * out_bytes]

    def scatter_importance(self, d_queries, d_coords, stream=None):  # -> shading.SCATTER_SAMPLE records
        return self._launch("crt_material_scatter_faces_n", d_queries, d_coords, 48, stream)

    def eval(self, d_queries, d_coords, stream=None):  # -> shading.BSDF_EVAL records
        return self._launch("crt_material_eval_faces_n", d_queries, d_coords, 32, stream)

    def emitted_directional(self, d_queries, stream=None):
        """The authored colour, as upstream (openpbr.rs:1211-1218): the untextured call."""
        return self.table.emitted_directional(d_queries, stream)
