"""The three builds of the deterministic math and the sampler behind one call shape (test infrastructure):

  oracle  oracle/ora_mathdrv.c in liboracle.so                    (ora_m_*)
  host    tests/host_shade/math_host.cpp: the device source, g++  (host_m_*)
  device  tests/host_shade/math_dev.hip: the device source, hipcc for gfx950, one kernel per function  (dev_m_*)

drv(name, *inputs) -> output array, or a tuple of them. C shape: (inputs..., size_t n, outputs...)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crust-render_amd", "csrc")
HOST_SHADE = os.path.join(ROOT, "tests", "host_shade")
HOST_FLAGS = ["-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes"]

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32
# name -> (inputs [(dtype, width)], outputs [(dtype, width)])
_U = lambda t: ([(t, 1)], [(t, 1)])
_B = lambda t: ([(t, 1), (t, 1)], [(t, 1)])
OPS = {
    "sincos": ([(f32, 1)], [(f32, 1), (f32, 1)]),
    "cos": _U(f32), "acos": _U(f32), "exp": _U(f32), "log": _U(f32),
    "pow": _B(f32), "rmax": _B(f32), "rmin": _B(f32), "smax": _B(f32), "smin": _B(f32),
    "rclamp": ([(f32, 1)] * 3, [(f32, 1)]),
    "pcg_hash": _U(u32), "laine_karras": _B(u32), "owen": _B(u32),
    "unit_f32": ([(u32, 1)], [(f32, 1)]),
    "sampler_new": ([(i32, 4)], [(u32, 1)]),
    "new_domain": ([(u32, 1), (i32, 1)], [(u32, 1)]),
    "draw_sample4": ([(u32, 1), (u32, 1)], [(f32, 4)]),
    "draw_rnd1": ([(u32, 1), (u32, 1)], [(f32, 1)]),
}
# the bare arithmetic: device source only (the oracle is plain C, there is nothing of its own to drive)
PRIMITIVES = {
    "add_f32": _B(f32), "sub_f32": _B(f32), "mul_f32": _B(f32), "div_f32": _B(f32), "sqrt_f32": _U(f32),
    "add_f64": _B(f64), "sub_f64": _B(f64), "mul_f64": _B(f64), "div_f64": _B(f64), "sqrt_f64": _U(f64),
    "f32_to_f64": ([(f32, 1)], [(f64, 1)]), "f64_to_f32": ([(f64, 1)], [(f32, 1)]), "rint_f64": _U(f64),
    "dot": ([(f32, 3), (f32, 3)], [(f32, 1)]), "normalize": ([(f32, 3)], [(f32, 3)]),
}
TABLE_WORDS = {"sobol_dirs": 4 * 32, "sobol_table": 3 * 4 * 256}


def _shape(n, w):
    return (n,) if w == 1 else (n, w)


class Driver:
    def __init__(self, lib, prefix, ops, device=False):
        self.lib, self.prefix, self.ops, self.device = lib, prefix, ops, device
        for name, (ins, outs) in ops.items():
            fn = getattr(lib, "%s_%s_n" % (prefix, name))
            fn.argtypes = [C.c_void_p] * len(ins) + [C.c_size_t] + [C.c_void_p] * len(outs)
            fn.restype = C.c_int if device else None
        for name in TABLE_WORDS:
            fn = getattr(lib, "%s_%s" % (prefix, name))
            fn.argtypes, fn.restype = [C.c_void_p], (C.c_int if device else None)

    def __call__(self, name, *args):
        ins, outs = self.ops[name]
        assert len(args) == len(ins), name
        arrs = [np.ascontiguousarray(a, dtype=t) for a, (t, w) in zip(args, ins)]
        n = arrs[0].shape[0]
        for a, (t, w) in zip(arrs, ins):
            assert a.shape == _shape(n, w), (name, a.shape, n, w)
        fn = getattr(self.lib, "%s_%s_n" % (self.prefix, name))
        if not self.device:
            res = [np.empty(_shape(n, w), dtype=t) for t, w in outs]
            fn(*[a.ctypes.data for a in arrs], n, *[r.ctypes.data for r in res])
        else:
            import torch
            d_in = [torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() for a in arrs]
            d_out = [torch.empty(int(np.prod(_shape(n, w))) * np.dtype(t).itemsize, dtype=torch.uint8, device="cuda")
                     for t, w in outs]
            torch.cuda.synchronize()
            err = fn(*[d.data_ptr() for d in d_in], n, *[d.data_ptr() for d in d_out])
            assert err == 0, "%s: hipError_t %d" % (name, err)
            res = [d.cpu().numpy().view(t).reshape(_shape(n, w)) for d, (t, w) in zip(d_out, outs)]
        return res[0] if len(res) == 1 else tuple(res)

    def table(self, name):
        fn = getattr(self.lib, "%s_%s" % (self.prefix, name))
        if not self.device:
            out = np.zeros(TABLE_WORDS[name], dtype=u32)
            fn(out.ctypes.data)
            return out
        import torch
        d = torch.zeros(TABLE_WORDS[name], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        err = fn(d.data_ptr())
        assert err == 0, "%s: hipError_t %d" % (name, err)
        return d.cpu().numpy().view(u32)


def oracle():
    import ora
    return Driver(ora.lib(), "ora_m", OPS)


def build_host(out_dir):
    """g++ over math_host.cpp exactly as tests/test_shading_seam_host.py builds seam_host.cpp -> path of the .so."""
    out = os.path.join(str(out_dir), "libmath_host.so")
    cmd = ["g++"] + HOST_FLAGS + ["-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(CSRC, "kernels"),
                                  "-I" + HOST_SHADE, os.path.join(HOST_SHADE, "math_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return out


def host(out_dir):
    return Driver(C.CDLL(build_host(out_dir)), "host_m", {**OPS, **PRIMITIVES})


def product_hipflags():
    """HIPFLAGS + KERNELFLAGS as csrc/Makefile holds them (paths in them are relative to csrc/)."""
    out = subprocess.run(["make", "-s", "-C", CSRC, "print-hipflags"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    flags = out.stdout.split()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags, flags
    return flags


def build_device(out_dir):
    """hipcc --offload-arch=gfx950 over math_dev.hip with the product's flags -> path of the .so. Needs no GPU."""
    out = os.path.join(str(out_dir), "libmath_dev.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + product_hipflags() + ["-shared", "-Ikernels", "-I" + HOST_SHADE,
                                          os.path.join(HOST_SHADE, "math_dev.hip"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=CSRC)
    assert res.returncode == 0, res.stderr[-3000:]
    return out


def device(out_dir):
    import torch  # first, so the HIP runtime the extension finds is the one torch has initialised
    assert torch.cuda.is_available()
    return Driver(C.CDLL(build_device(out_dir)), "dev_m", {**OPS, **PRIMITIVES}, device=True)
