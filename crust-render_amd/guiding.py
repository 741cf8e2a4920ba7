"""The path guiding field as callable device functions — host mirror of `GuidingField` (crates/crust-core/src/guiding/
field.rs:57-113 over sdtree.rs and dtree.rs) behind the C ABI (include/crt_guiding.h: crt_guiding_new / _free / _update /
_image / _stats, crt_guiding_sample_n, crt_guiding_pdf_n, crt_material_scatter_guided_n).

A host integrator that keeps its own trace_path records one SAMPLE per path vertex during a training pass, calls `update`
between passes (host arithmetic, single-threaded: the f32 sums depend on the order) and queries `sample` / `pdf` — or the
whole bounce, shading.DeviceMaterials.scatter_guided — while tracing. Query and result records live
in HBM as torch uint8 tensors; numpy structured dtypes give them field names on the host. There is no CPU fallback:
sample, pdf and the guided bounce launch kernels of libcrt_amd.so. Building and updating the field, reading its image and
its tallies need no device. The wavefront renderer reads a field only where one is bound to it
(Renderer.set_guiding: the guided pass of render_guided; the renderer trains nothing — the field's owner does).
"""
import ctypes as C

import numpy as np

MAX_DTREE_DEPTH, MAX_SPATIAL_DEPTH, MIN_RHO = 32, 32, 1.0 / 1024.0
NO_CHILD = LEAF = 0xFFFFFFFF
FLAG_TRAINED, FLAG_FROM_GUIDE = 4, 8  # SCATTER_SAMPLE flags bits 2 and 3 of scatter_guided

_f, _u = np.float32, np.uint32
CONFIG = np.dtype([("train_iterations", _u), ("guide_prob", _f), ("spatial_c", _f), ("dtree_rho", _f),
                   ("dtree_max_depth", _u), ("spatial_max_depth", _u)])
SAMPLE = np.dtype([("pos", _f, 3), ("radiance", _f), ("dir", _f, 3), ("_pad", _u)])
QUERY = np.dtype([("pos", _f, 3), ("seed_u", _f), ("dir", _f, 3), ("seed_v", _f)])
RESULT = np.dtype([("dir", _f, 3), ("pdf", _f), ("some", _u), ("trained", _u), ("_pad", _u, 2)])
STATS = np.dtype([("s_nodes", _u), ("s_leaves", _u), ("s_depth", _u), ("d_trees", _u), ("d_nodes", _u), ("d_depth", _u),
                  ("recorded", np.uint64)])
# the image crt_guiding_image hands out (csrc/kernels/guiding.hip.h: GuideHeader, GuideSNode, GuideDNode)
IMAGE_HEADER = np.dtype([("magic", _u), ("bytes", _u), ("bmin", _f, 3), ("bmax", _f, 3), ("alpha", _f), ("off_snodes", _u),
                         ("n_snodes", _u), ("off_dnodes", _u), ("n_dnodes", _u), ("n_dtrees", _u), ("s_depth", _u),
                         ("d_depth", _u), ("_pad", _u, 48)])
IMAGE_SNODE = np.dtype([("axis", _u), ("split", _f), ("a", _u), ("b", _u)])
IMAGE_DNODE = np.dtype([("sums", _f, 4), ("children", _u, 4)])
assert (CONFIG.itemsize, SAMPLE.itemsize, QUERY.itemsize, RESULT.itemsize, STATS.itemsize) == (24, 32, 32, 32, 32)
assert (IMAGE_HEADER.itemsize, IMAGE_SNODE.itemsize, IMAGE_DNODE.itemsize) == (256, 16, 32)
MAGIC = 0x44475243


def _crt():
    import sys
    return sys.modules[__name__.rsplit(".", 1)[0]]


class GuidingConfig:
    """GuidingConfig (field.rs:13-41) with its defaults. guide_prob is handed on as given: the clamp to [0.1, 0.9] is
    with_guiding's (tracer.rs:696-700) and the importer's (usda.load(path_guiding=True))."""

    def __init__(self, train_iterations=4, guide_prob=0.5, spatial_c=4000.0, dtree_rho=0.01, dtree_max_depth=20,
                 spatial_max_depth=24):
        self.train_iterations, self.guide_prob, self.spatial_c = int(train_iterations), float(guide_prob), float(spatial_c)
        self.dtree_rho, self.dtree_max_depth, self.spatial_max_depth = float(dtree_rho), int(dtree_max_depth), int(spatial_max_depth)

    def record(self):
        r = np.zeros(1, CONFIG)
        for name in CONFIG.names:
            r[name] = getattr(self, name)
        return r

    @classmethod
    def default(cls):
        """crt_guiding_config_default's answer."""
        r = np.zeros(1, CONFIG)
        _crt().lib().crt_guiding_config_default(C.c_void_p(r.ctypes.data))
        return cls(**{name: r[name][0].item() for name in CONFIG.names})


def to_device(records, device="cuda:0"):
    """numpy array -> torch uint8 tensor in HBM."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).to(device)


def samples(pos, direction, radiance):
    """SAMPLE records from arrays: positions [n, 3], directions [n, 3], radiance [n]."""
    radiance = np.asarray(radiance, _f).reshape(-1)
    out = np.zeros(len(radiance), SAMPLE)
    out["pos"], out["dir"], out["radiance"] = np.asarray(pos, _f), np.asarray(direction, _f), radiance
    return out


class GuidingField:
    """GuidingField::new over crt_guiding_new: the bounds are padded as upstream pads them. Host only until sample / pdf /
    scatter_guided first run. Raises CrtError with the library's reason when the configuration is refused."""

    def __init__(self, bounds_min, bounds_max, cfg=None):
        crt = _crt()
        self.cfg = cfg if cfg is not None else GuidingConfig()
        lo, hi = np.asarray(bounds_min, _f).reshape(3).copy(), np.asarray(bounds_max, _f).reshape(3).copy()
        rec = self.cfg.record()
        self.h = crt.lib().crt_guiding_new(crt._fp(lo), crt._fp(hi), C.c_void_p(rec.ctypes.data))
        if not self.h:
            raise crt.CrtError(-1, "crt_guiding_new")

    @classmethod
    def for_scene(cls, scene, cfg=None):
        """The field over a committed scene's bounds (crt_scene_bounds), as render_guided builds it (tracer.rs:245-262)."""
        b = scene.bounds()  # crt_scene_bounds: min then max, None for an empty scene
        if b is None:
            raise ValueError("GuidingField.for_scene: the scene is empty, it has no bounds")
        return cls(b[:3], b[3:], cfg)

    def close(self):
        """Drops the handle now (crt_guiding_free); the object is unusable afterwards."""
        h, self.h = getattr(self, "h", None), None
        if h:
            _crt().lib().crt_guiding_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, sample_records, next_iteration):
        """GuidingField::update (field.rs:101-112): SAMPLE records on the HOST, splat in array order, then both refines.
        No guiding launch may be in flight on another stream."""
        crt = _crt()
        s = np.ascontiguousarray(sample_records, dtype=SAMPLE)
        crt._check(crt.lib().crt_guiding_update(self.h, C.c_void_p(s.ctypes.data if len(s) else 0), len(s), int(next_iteration)),
                   "crt_guiding_update")

    def image_bytes(self):
        """The image the kernels read (crt_guiding_image), as a numpy uint8 copy."""
        crt = _crt()
        p, n = C.c_void_p(), C.c_size_t()
        crt._check(crt.lib().crt_guiding_image(self.h, C.byref(p), C.byref(n)), "crt_guiding_image")
        return np.frombuffer(C.string_at(p.value, n.value), np.uint8).copy()

    def image(self):
        """The image's parts: (header record, IMAGE_SNODE records, IMAGE_DNODE records)."""
        raw = self.image_bytes()
        hd = raw[:256].view(IMAGE_HEADER)[0]
        s = raw[hd["off_snodes"]:hd["off_snodes"] + 16 * int(hd["n_snodes"])].view(IMAGE_SNODE)
        d = raw[hd["off_dnodes"]:hd["off_dnodes"] + 32 * int(hd["n_dnodes"])].view(IMAGE_DNODE)
        return hd, s.copy(), d.copy()

    def stats(self):
        """crt_guiding_stats as a dict."""
        crt = _crt()
        st = np.zeros(1, STATS)
        crt._check(crt.lib().crt_guiding_stats(self.h, C.c_void_p(st.ctypes.data)), "crt_guiding_stats")
        return {name: int(st[name][0]) for name in STATS.names}

    def _query(self, fn, d_queries, stream):
        import torch
        crt = _crt()
        n = d_queries.numel() * d_queries.element_size() // QUERY.itemsize
        d_out = torch.empty(max(n * RESULT.itemsize, 1), dtype=torch.uint8, device=d_queries.device)
        crt._check(getattr(crt.lib(), fn)(self.h, C.c_void_p(d_queries.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                          crt._stream_ptr(stream)), fn)
        return d_out[:n * RESULT.itemsize]

    def sample(self, d_queries, stream=None):
        """GuidingField::sample (field.rs:88-91): QUERY records (pos, seed_u, seed_v; uint8 device tensor) -> RESULT records."""
        return self._query("crt_guiding_sample_n", d_queries, stream)

    def pdf(self, d_queries, stream=None):
        """GuidingField::pdf (field.rs:95-97): QUERY records (pos, dir) -> RESULT records (pdf, trained)."""
        return self._query("crt_guiding_pdf_n", d_queries, stream)
