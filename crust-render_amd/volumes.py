"""Volume regions as callable device functions — host mirror of `Volumes` (crates/crust-core/src/volume.rs:356-537) over
the C ABI's batched entry points (include/crt.h: crt_volumes_new / _free / _image, crt_volumes_density_n,
crt_volumes_transmittance_n, crt_volumes_sample_n).

A host integrator that keeps its own trace_path (tracer.rs:1167-1254) calls Scene.intersect_n / occluded_n for the kernel
seam, shading.py for the per-hit shading and these for fog and smoke: `sample` at every path segment, `transmittance` on
shadow rays. The wavefront renderer runs the same functions itself once an aggregate is bound to it
(Renderer.set_volumes). Query and result records live in HBM as torch uint8
tensors; numpy structured dtypes give them field names on the host. There is no CPU fallback: density, transmittance and
sample launch kernels of libcrt_amd.so. Building the aggregate and reading its image need no device.
"""
import ctypes as C

import numpy as np

MAX_STEPS, MAX_REGIONS, MAX_OCTAVES = 65536, 8, 32
HOMOGENEOUS, NOISE, GRID = 0, 1, 2
OK, STEP_LIMIT = 0, 1
PASSTHROUGH, SCATTER = 0, 1
FIELDS = {"homogeneous": HOMOGENEOUS, "noise": NOISE, "smoke": NOISE, "grid": GRID}

_f, _u = np.float32, np.uint32
REGION = np.dtype([("local_to_world", _f, 12), ("half_extent", _f, 3), ("sigma_s", _f, 3), ("sigma_a", _f, 3), ("g", _f),
                   ("emission", _f, 3), ("density_scale", _f), ("field", _u), ("noise_scale", _f), ("noise_octaves", _u),
                   ("noise_gain", _f), ("noise_lacunarity", _f), ("noise_threshold", _f), ("noise_seed", _u),
                   ("grid_dims", _u, 3), ("grid_offset", _u), ("grid_count", _u)])
QUERY = np.dtype([("origin", _f, 3), ("t_eps", _f), ("direction", _f, 3), ("t_max", _f), ("seed", _u), ("_pad", _u, 3)])
TRANSMITTANCE = np.dtype([("transmittance", _f, 3), ("status", _u)])
EVENT = np.dtype([("p", _f, 3), ("t", _f), ("weight", _f, 3), ("kind", _u), ("emitted", _f, 3), ("n_lobes", _u),
                  ("dir", _f, 3), ("pdf", _f), ("lobes", _f, (MAX_REGIONS, 2)), ("status", _u), ("_pad", _u, 3)])
# the image crt_volumes_image hands out (csrc/kernels/volume.hip.h: VolHeader, VolRegionRec)
IMAGE_HEADER = np.dtype([("magic", _u), ("n_regions", _u), ("region_bytes", _u), ("off_regions", _u), ("off_grid", _u),
                         ("grid_floats", _u), ("bytes", _u), ("_pad", _u, 57)])
IMAGE_REGION = np.dtype([("w2l", _f, 12), ("half", _f, 3), ("majorant", _f), ("bmin", _f, 3), ("field", _u), ("bmax", _f, 3),
                         ("g", _f), ("sigma_s", _f, 3), ("noise_scale", _f), ("sigma_a", _f, 3), ("noise_gain", _f),
                         ("emission", _f, 3), ("noise_lacunarity", _f), ("noise_threshold", _f), ("noise_octaves", _u),
                         ("noise_seed", _u), ("grid_off", _u), ("nx", _u), ("ny", _u), ("nz", _u), ("_pad", _u)])
assert (REGION.itemsize, QUERY.itemsize, TRANSMITTANCE.itemsize, EVENT.itemsize) == (152, 48, 16, 144)
assert (IMAGE_HEADER.itemsize, IMAGE_REGION.itemsize) == (256, 176)
IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=_f)


def _crt():
    import sys
    return sys.modules[__name__.rsplit(".", 1)[0]]


def region(local_to_world=None, half_extent=0.5, sigma_s=0.5, sigma_a=0.0, g=0.0, emission=0.0, density_scale=1.0,
           field="homogeneous", noise_scale=4.0, noise_octaves=4, noise_gain=0.5, noise_lacunarity=2.0, noise_threshold=0.3,
           noise_seed=0, grid_dims=None, grid_data=None):
    """The arguments of VolumeRegion::new as a dict (the importer's defaults, usd_import.rs:435-505). Colours and the
    half extent take a scalar or three values; field is "homogeneous", "noise" ("smoke") or "grid"."""
    return dict(local_to_world=local_to_world, half_extent=half_extent, sigma_s=sigma_s, sigma_a=sigma_a, g=g, emission=emission,
                density_scale=density_scale, field=field, noise_scale=noise_scale, noise_octaves=noise_octaves,
                noise_gain=noise_gain, noise_lacunarity=noise_lacunarity, noise_threshold=noise_threshold,
                noise_seed=noise_seed, grid_dims=grid_dims, grid_data=grid_data)


def pack_regions(regions):
    """Dicts (see region()) -> (REGION record array, one float32 grid array). A REGION array with its grid passes through:
    pack_regions((records, grid))."""
    if isinstance(regions, tuple) and isinstance(regions[0], np.ndarray) and regions[0].dtype == REGION:
        grid = regions[1]
        return np.ascontiguousarray(regions[0]), np.ascontiguousarray(grid if grid is not None else np.zeros(0), dtype=_f)
    out = np.zeros(len(regions), REGION)
    grids, offset = [], 0
    for r, d in zip(out, regions):
        d = dict(region(), **d)
        m = d["local_to_world"]
        r["local_to_world"] = IDENTITY12 if m is None else np.asarray(m, _f).reshape(12)
        for key in ("half_extent", "sigma_s", "sigma_a", "emission"):
            r[key] = np.broadcast_to(np.asarray(d[key], _f), 3)
        for key in ("g", "density_scale", "noise_scale", "noise_gain", "noise_lacunarity", "noise_threshold"):
            r[key] = d[key]
        field = d["field"]
        r["field"] = FIELDS[field] if isinstance(field, str) else int(field)
        r["noise_octaves"] = int(d["noise_octaves"])
        r["noise_seed"] = int(d["noise_seed"]) & 0xFFFFFFFF
        if d["grid_dims"] is not None or d["grid_data"] is not None:
            data = np.asarray(d["grid_data"] if d["grid_data"] is not None else [], _f).reshape(-1)
            r["grid_dims"] = np.asarray(d["grid_dims"] if d["grid_dims"] is not None else (0, 0, 0), np.int64).reshape(3)
            r["grid_offset"], r["grid_count"] = offset, data.size
            grids.append(data)
            offset += data.size
    return out, (np.concatenate(grids) if grids else np.zeros(0, _f))


def to_device(records, device="cuda:0"):
    """numpy array -> torch uint8 tensor in HBM."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).to(device)


class Volumes:
    """Volumes::new over crt_volumes_new: regions as dicts (region()) or as (REGION records, grid floats). Host only
    until density / transmittance / sample first run. Raises CrtError with the library's reason when the aggregate is
    refused (more than MAX_REGIONS regions, a non-finite field, a grid whose dims do not match its data, a singular
    placement)."""

    def __init__(self, regions):
        crt = _crt()
        self.records, self.grid = pack_regions(regions)
        self.n = len(self.records)
        L = crt.lib()
        self.h = L.crt_volumes_new(C.c_void_p(self.records.ctypes.data if self.n else 0), self.n,
                                   crt._fp(self.grid) if self.grid.size else None, self.grid.size)
        if not self.h:
            raise crt.CrtError(-1, "crt_volumes_new")

    def close(self):
        """Drops the handle now (crt_volumes_free); the object is unusable afterwards."""
        h, self.h = getattr(self, "h", None), None
        if h:
            _crt().lib().crt_volumes_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image_bytes(self):
        """The image the kernels read (crt_volumes_image), as a numpy uint8 copy."""
        crt = _crt()
        p, n = C.c_void_p(), C.c_size_t()
        crt._check(crt.lib().crt_volumes_image(self.h, C.byref(p), C.byref(n)), "crt_volumes_image")
        return np.frombuffer(C.string_at(p.value, n.value), np.uint8).copy()

    def image(self):
        """The image's parts: (header record, IMAGE_REGION records [n], grid floats)."""
        raw = self.image_bytes()
        hd = raw[:256].view(IMAGE_HEADER)[0]
        recs = raw[hd["off_regions"]:hd["off_regions"] + MAX_REGIONS * IMAGE_REGION.itemsize].view(IMAGE_REGION)[:hd["n_regions"]]
        grid = raw[hd["off_grid"]:hd["off_grid"] + 4 * int(hd["grid_floats"])].view(_f)
        return hd, recs.copy(), grid.copy()

    def density(self, region, d_points, stream=None):
        """VolumeRegion::density (volume.rs:234-242): float32 device tensor [n, 3] -> float32 device tensor [n]."""
        import torch
        crt = _crt()
        n = d_points.numel() // 3
        d_out = torch.empty(max(n, 1), dtype=torch.float32, device=d_points.device)
        crt._check(crt.lib().crt_volumes_density_n(self.h, int(region), C.c_void_p(d_points.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                                  crt._stream_ptr(stream)), "crt_volumes_density_n")
        return d_out[:n]

    def transmittance(self, d_queries, stream=None):
        """Volumes::transmittance (volume.rs:492-536): QUERY records (uint8 device tensor) -> TRANSMITTANCE records."""
        import torch
        crt = _crt()
        n = d_queries.numel() * d_queries.element_size() // QUERY.itemsize
        d_out = torch.empty(max(n * TRANSMITTANCE.itemsize, 1), dtype=torch.uint8, device=d_queries.device)
        crt._check(crt.lib().crt_volumes_transmittance_n(self.h, C.c_void_p(d_queries.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                                        crt._stream_ptr(stream)), "crt_volumes_transmittance_n")
        return d_out[:n * TRANSMITTANCE.itemsize]

    def sample(self, d_queries, d_phase_u=None, stream=None):
        """Volumes::sample_interaction (volume.rs:409-486): QUERY records -> EVENT records. d_phase_u: float32 device
        tensor [n, 3] (lobe_u, hg_u, hg_v); with it a scatter also carries PhaseMix::sample's direction and
        max(PhaseMix::pdf, 1e-6) (tracer.rs:1193-1196)."""
        import torch
        crt = _crt()
        n = d_queries.numel() * d_queries.element_size() // QUERY.itemsize
        d_out = torch.empty(max(n * EVENT.itemsize, 1), dtype=torch.uint8, device=d_queries.device)
        crt._check(crt.lib().crt_volumes_sample_n(self.h, C.c_void_p(d_queries.data_ptr()),
                                                 C.c_void_p(d_phase_u.data_ptr() if d_phase_u is not None else 0), n,
                                                 C.c_void_p(d_out.data_ptr()), crt._stream_ptr(stream)), "crt_volumes_sample_n")
        return d_out[:n * EVENT.itemsize]
