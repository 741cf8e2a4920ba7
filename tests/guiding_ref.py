"""A float32 numpy restatement of the path guiding field — crates/crust-core/src/guiding/{mod,dtree,sdtree,field}.rs:
record, the two refines, the split, sample, pdf and the two maps — written from the Rust text, one numpy operation per
reference operation, independent of csrc/guiding.cpp and csrc/kernels/guiding.hip.h. The truth of tests/test_guiding.py
(the library's image after every update, the device source compiled for the host) and tests/test_gpu_guiding.py (the
kernels), in the style of tests/env_ref.py and tests/volume_ref.py.

Vectorised over samples and queries, never over a sum: DTree::record adds one sample at a time, and an f32 accumulator
depends on the order, so a training pass is replayed per accumulator (node, quadrant) with np.add.accumulate — a strictly
sequential float32 running sum — over the fluxes in array order.

What is NOT restated: cos / sin / atan2. Upstream calls libm; the project calls its own deterministic sincos_det /
atan2_det (kernels/dmath.hip.h, pinned by tests/test_math_host.py), and this file takes those two from the device source
compiled for the host (tests/host_shade/guiding_host.cpp: host_guide_sincos_n, host_guide_atan2_n) — so the bits stated
here are device == restatement, and statistically against upstream's unit tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crust-render_amd", "csrc")
HOST_SHADE = os.path.join(ROOT, "tests", "host_shade")
HOST_FLAGS = ["-std=c++17", "-O1", "-fPIC", "-shared", "-fno-fast-math", "-Wno-attributes"]

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
NO_CHILD = 0xFFFFFFFF
ONE_MINUS_EPS = f32(1.0) - f32(np.finfo(np.float32).eps)  # dtree.rs:15
PI, TAU = f32(np.pi), f32(2.0 * np.pi)                    # std::f32::consts
INV_4PI = f32(1.0) / (f32(4.0) * PI)                       # dtree.rs:130

SAMPLE = np.dtype([("pos", f32, 3), ("radiance", f32), ("dir", f32, 3), ("_pad", u32)])
QUERY = np.dtype([("pos", f32, 3), ("seed_u", f32), ("dir", f32, 3), ("seed_v", f32)])
RESULT = np.dtype([("dir", f32, 3), ("pdf", f32), ("some", u32), ("trained", u32), ("_pad", u32, 2)])


# ---- the device source compiled for the host: the twin under test AND the source of sincos / atan2 ---------------------
class Host:
    def __init__(self, out_dir, contract="off"):
        out = os.path.join(str(out_dir), "libguiding_host_%s.so" % contract)
        # "fast": the build that must FAIL the bit comparison — FMA contraction allowed (g++ forms FMAs from -O2 on)
        cmd = ["g++"] + HOST_FLAGS + ["-ffp-contract=" + contract] + (["-O2", "-mfma"] if contract == "fast" else []) + [
            "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(CSRC, "kernels"),
            os.path.join(HOST_SHADE, "guiding_host.cpp"), "-o", out]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        self.lib = C.CDLL(out)

    def _call(self, name, *args):
        fn = getattr(self.lib, name)
        fn.restype = None
        fn(*[C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in args])

    def sincos(self, x):
        x = np.ascontiguousarray(x, f32)
        s, c = np.zeros_like(x), np.zeros_like(x)
        self._call("host_guide_sincos_n", x, C.c_size_t(x.size), s, c)
        return s, c

    def atan2(self, y, x):
        y, x = np.ascontiguousarray(y, f32), np.ascontiguousarray(x, f32)
        o = np.zeros_like(x)
        self._call("host_guide_atan2_n", y, x, C.c_size_t(x.size), o)
        return o

    def dir_to_canonical(self, d):
        d = np.ascontiguousarray(d, f32).reshape(-1, 3)
        o = np.zeros((len(d), 2), f32)
        self._call("host_guide_dir_to_canonical_n", d, C.c_size_t(len(d)), o)
        return o

    def canonical_to_dir(self, p):
        p = np.ascontiguousarray(p, f32).reshape(-1, 2)
        o = np.zeros((len(p), 3), f32)
        self._call("host_guide_canonical_to_dir_n", p, C.c_size_t(len(p)), o)
        return o

    def pcg(self, state, n):
        o = np.zeros(n, f32)
        self._call("host_guide_pcg_n", C.c_uint64(int(state)), C.c_size_t(n), o)
        return o

    def luminance(self, c):
        c = np.ascontiguousarray(c, f32).reshape(-1, 3)
        o = np.zeros(len(c), f32)
        self._call("host_guide_luminance_n", c, C.c_size_t(len(c)), o)
        return o

    def dtree_sample(self, image, pos, seeds):
        """DTree::sample of the tree governing `pos`: seeds [n, 2] -> (canonical points [n, 2], pdf [n], some [n])."""
        image, seeds = np.ascontiguousarray(image), np.ascontiguousarray(seeds, f32).reshape(-1, 2)
        pos = np.ascontiguousarray(pos, f32)
        p, pdf, some = np.zeros((len(seeds), 2), f32), np.zeros(len(seeds), f32), np.zeros(len(seeds), u32)
        self._call("host_guide_dtree_sample_n", image, pos, seeds, C.c_size_t(len(seeds)), p, pdf, some)
        return p, pdf, some

    def dtree_pdf(self, image, pos, p):
        image, p, pos = np.ascontiguousarray(image), np.ascontiguousarray(p, f32).reshape(-1, 2), np.ascontiguousarray(pos, f32)
        pdf = np.zeros(len(p), f32)
        self._call("host_guide_dtree_pdf_n", image, pos, p, C.c_size_t(len(p)), pdf)
        return pdf

    def _query(self, name, image, q):
        image, q = np.ascontiguousarray(image), np.ascontiguousarray(q)
        out = np.zeros(len(q), RESULT)
        self._call(name, image, q, C.c_size_t(len(q)), out)
        return out

    def sample(self, image, q): return self._query("host_guide_sample_n", image, q)
    def pdf(self, image, q): return self._query("host_guide_pdf_n", image, q)

    def scatter(self, image, mats, q, out_dtype):
        image, mats, q = np.ascontiguousarray(image), np.ascontiguousarray(mats), np.ascontiguousarray(q)
        out = np.zeros(len(q), out_dtype)
        self._call("host_guide_scatter_n", image, mats, C.c_size_t(len(mats)), q, C.c_size_t(len(q)), out)
        return out

    def plain_scatter(self, mats, q, out_dtype):
        mats, q = np.ascontiguousarray(mats), np.ascontiguousarray(q)
        out = np.zeros(len(q), out_dtype)
        self._call("host_guide_plain_scatter_n", mats, C.c_size_t(len(mats)), q, C.c_size_t(len(q)), out)
        return out


_HOSTS = {}


def host(out_dir, contract="off"):
    """One build per directory and contraction mode (a module-scoped tmp dir in the tests)."""
    key = (str(out_dir), contract)
    if key not in _HOSTS:
        _HOSTS[key] = Host(out_dir, contract)
    return _HOSTS[key]


# ---- scalar helpers with the reference's operand semantics --------------------------------------------------------------
def rclamp(x, lo, hi):  # f32::clamp: a NaN passes through
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(f32)


def rmax(a, b):  # f32::max: a NaN operand yields the other one
    return np.where((a > b) | np.isnan(b), a, b).astype(f32)


def luminance(c):  # guiding/mod.rs:18-20
    c = np.asarray(c, f32).reshape(-1, 3)
    return (f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1]) + f32(0.0722) * c[:, 2]


def pcg_f32(state):  # dtree.rs:19-27 on an array of u64 states: (new states, uniforms)
    with np.errstate(over="ignore"):
        state = state * u64(6364136223846793005) + u64(1442695040888963407)
    xorshifted = (((state >> u64(18)) ^ state) >> u64(27)).astype(u32)
    rot = (state >> u64(59)).astype(u32)
    bits = (xorshifted >> rot) | (xorshifted << ((u32(32) - rot) & u32(31)))
    return state, (bits >> u32(8)).astype(f32) * f32(1.0 / 16777216.0)


def quadrant(p0, p1):  # dtree.rs:48-56
    qx, qy = p0 >= f32(0.5), p1 >= f32(0.5)
    c0 = rclamp(p0 * f32(2.0) - qx.astype(f32), f32(0.0), ONE_MINUS_EPS)
    c1 = rclamp(p1 * f32(2.0) - qy.astype(f32), f32(0.0), ONE_MINUS_EPS)
    return qx.astype(np.int64) + 2 * qy.astype(np.int64), c0, c1


class Maps:
    """dir_to_canonical / canonical_to_dir (dtree.rs:30-43) over the deterministic atan2 / sincos of a Host."""

    def __init__(self, h):
        self.h = h

    def dir_to_canonical(self, d):
        d = np.asarray(d, f32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])  # the project's normalize
            x, y, z = d[:, 0] / length, d[:, 1] / length, d[:, 2] / length
            u = self.h.atan2(y, x) / TAU + f32(0.5)
            v = (z + f32(1.0)) * f32(0.5)
        return rclamp(u, f32(0.0), ONE_MINUS_EPS), rclamp(v, f32(0.0), ONE_MINUS_EPS)

    def canonical_to_dir(self, p0, p1):
        with np.errstate(all="ignore"):
            phi = TAU * (p0 - f32(0.5))
            z = f32(2.0) * p1 - f32(1.0)
            r = np.sqrt(rmax(f32(1.0) - z * z, np.zeros_like(z)))
            s, c = self.h.sincos(phi)
            return np.stack([r * c, r * s, z], axis=1).astype(f32)


# ---- DTree (dtree.rs) --------------------------------------------------------------------------------------------------
class DTree:
    def __init__(self):
        self.sums = np.zeros((1, 4), f32)
        self.children = np.full((1, 4), NO_CHILD, np.int64)

    def copy(self):
        t = DTree()
        t.sums, t.children = self.sums.copy(), self.children.copy()
        return t

    @staticmethod
    def total(s):  # DNode::total, dtree.rs:76-78
        return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]

    def total_flux(self):
        return self.total(self.sums[0])

    def record(self, p0, p1, flux):
        """dtree.rs:106-121 for a batch, in array order: one sequential f32 running sum per (node, quadrant)."""
        with np.errstate(invalid="ignore"):
            keep = np.isfinite(flux) & (flux > 0)
        p0, p1, flux = p0[keep], p1[keep], flux[keep]
        order = np.arange(len(flux))
        node = np.zeros(len(flux), np.int64)
        keys, vals, idx = [], [], []
        while len(order):
            q, c0, c1 = quadrant(p0, p1)
            keys.append(node * 4 + q); vals.append(flux); idx.append(order)
            child = self.children[node, q]
            go = child != NO_CHILD
            node, p0, p1, flux, order = child[go], c0[go], c1[go], flux[go], order[go]
        if not keys:
            return
        keys, vals, idx = np.concatenate(keys), np.concatenate(vals), np.concatenate(idx)
        by = np.lexsort((idx, keys))  # per accumulator, in sample order
        keys, vals = keys[by], vals[by]
        starts = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0]
        ends = np.r_[starts[1:], len(keys)]
        flat = self.sums.reshape(-1)
        for a, b in zip(starts, ends):
            k = keys[a]
            flat[k] = np.add.accumulate(np.r_[flat[k], vals[a:b]].astype(f32), dtype=f32)[-1]

    def refine(self, rho, max_depth):  # dtree.rs:226-275
        sums, children = [np.zeros(4, f32)], [[NO_CHILD] * 4]
        total = self.total_flux()
        if total <= 0:
            return DTree()

        def rec(out_idx, old_idx, seeded, depth):
            s = self.sums[old_idx].copy() if old_idx is not None else seeded
            sums[out_idx] = s
            for q in range(4):
                flux = s[q]
                if flux > rho * total and depth < max_depth:
                    child_idx = len(sums)
                    sums.append(np.zeros(4, f32)); children.append([NO_CHILD] * 4)
                    children[out_idx][q] = child_idx
                    old_child = None
                    if old_idx is not None and self.children[old_idx, q] != NO_CHILD:
                        old_child = int(self.children[old_idx, q])
                    rec(child_idx, old_child, np.full(4, flux / f32(4.0), f32), depth + 1)

        rec(0, 0, None, 1)
        out = DTree()
        out.sums, out.children = np.array(sums, f32).reshape(-1, 4), np.array(children, np.int64).reshape(-1, 4)
        return out

    def depth(self, idx=0):  # dtree.rs:280-291
        d = 1
        for c in self.children[idx]:
            if c != NO_CHILD:
                d = max(d, 1 + self.depth(int(c)))
        return d


# ---- the flattened trees: what sample / pdf descend, and what the image must equal ---------------------------------------
class Flat:
    """S-nodes as (axis | 0xFFFFFFFF, split, a, b) and every D-tree in one array with absolute child indices — the image's
    content (csrc/kernels/guiding.hip.h), built here from the restatement's own trees."""

    def __init__(self, field):
        self.bmin, self.bmax, self.alpha = field.bmin, field.bmax, f32(field.cfg["guide_prob"])
        roots, at = [], 0
        for t in field.dtrees:
            roots.append(at); at += len(t.sums)
        self.sums = np.concatenate([t.sums for t in field.dtrees]).astype(f32)
        self.children = np.concatenate([np.where(t.children == NO_CHILD, NO_CHILD, t.children + r)
                                        for t, r in zip(field.dtrees, roots)]).astype(np.int64)
        n = len(field.nodes)
        self.axis, self.split = np.zeros(n, np.int64), np.zeros(n, f32)
        self.a, self.b = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i, nd in enumerate(field.nodes):
            if nd["leaf"]:
                self.axis[i], self.a[i] = NO_CHILD, roots[nd["dtree"]]
            else:
                self.axis[i], self.split[i], self.a[i], self.b[i] = nd["axis"], nd["split"], nd["children"][0], nd["children"][1]
        self.roots = np.array(roots, np.int64)

    def dtree_at(self, pos):  # sdtree.rs:43-66 -> the root node of the governing D-tree
        pos = np.asarray(pos, f32).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            p = np.where(pos > self.bmin, pos, self.bmin)  # glam clamp: maxps, then minps
            p = np.where(p < self.bmax, p, self.bmax).astype(f32)
            node = np.zeros(len(p), np.int64)
            while True:
                inner = self.axis[node] != NO_CHILD
                if not inner.any():
                    return self.a[node]
                ax = np.where(inner, self.axis[node], 0)
                right = p[np.arange(len(p)), ax] >= self.split[node]
                node = np.where(inner, np.where(right, self.b[node], self.a[node]), node)

    def trained_at(self, pos):  # field.rs:81-83
        return DTree.total(self.sums[self.dtree_at(pos)]) > 0

    def dtree_pdf(self, root, p0, p1):  # dtree.rs:125-151
        n = len(root)
        out = np.zeros(n, f32)
        with np.errstate(all="ignore"):
            live = ~(DTree.total(self.sums[root]) <= 0)  # total_flux() <= 0.0 -> 0.0
            idx = np.nonzero(live)[0]
            node, p0, p1 = root[idx], p0[idx].copy(), p1[idx].copy()
            pdf = np.full(len(idx), INV_4PI, f32)
            while len(idx):
                s = self.sums[node]
                total = DTree.total(s)
                done = total <= 0  # no information below this node: uniform over its domain
                q, c0, c1 = quadrant(p0, p1)
                frac = s[np.arange(len(idx)), q] / total
                zero = ~done & (frac <= 0)
                step = ~done & ~zero
                pdf = np.where(step, pdf * (f32(4.0) * frac), pdf).astype(f32)
                child = self.children[node, q]
                end = done | zero | (child == NO_CHILD)
                out[idx[end]] = np.where(zero, f32(0.0), pdf)[end]
                go = ~end
                idx, node, p0, p1, pdf = idx[go], child[go], c0[go], c1[go], pdf[go]
        return out

    def dtree_sample(self, root, seed_u, seed_v):  # dtree.rs:163-219 -> some, p0, p1, pdf
        n = len(root)
        with np.errstate(all="ignore"):
            some = ~(DTree.total(self.sums[root]) <= 0)
            state = ((seed_u.view(u32).astype(u64) << u64(32)) | seed_v.view(u32).astype(u64)) ^ u64(0x9E3779B97F4A7C15)
            base0, base1 = np.zeros(n, f32), np.zeros(n, f32)
            scale, pdf = np.ones(n, f32), np.full(n, INV_4PI, f32)
            node, act = root.copy(), some.copy()
            while act.any():
                s = self.sums[node]
                total = DTree.total(s)
                act = act & ~(total <= 0)  # break: uniform within its domain
                st, u0 = pcg_f32(state)
                st, u1 = pcg_f32(st)
                state = np.where(act, st, state)
                p_left = (s[:, 0] + s[:, 2]) / total
                qx = (u0 >= p_left).astype(np.int64)
                rows = np.arange(n)
                col_total = s[rows, qx] + s[rows, qx + 2]
                p_bottom = np.where(col_total > 0, s[rows, qx] / col_total, f32(0.5)).astype(f32)
                qy = (u1 >= p_bottom).astype(np.int64)
                q = qx + 2 * qy
                frac = s[rows, q] / total
                act = act & ~(frac <= 0)  # break: numerically unreachable quadrant
                pdf = np.where(act, pdf * (f32(4.0) * frac), pdf).astype(f32)
                base0 = np.where(act, base0 + f32(0.5) * scale * qx.astype(f32), base0).astype(f32)
                base1 = np.where(act, base1 + f32(0.5) * scale * qy.astype(f32), base1).astype(f32)
                scale = np.where(act, scale * f32(0.5), scale).astype(f32)
                child = self.children[node, q]
                act = act & (child != NO_CHILD)
                node = np.where(act, child, node)
            state, u0 = pcg_f32(state)
            state, u1 = pcg_f32(state)
            p0 = rclamp(base0 + u0 * scale, f32(0.0), ONE_MINUS_EPS)
            p1 = rclamp(base1 + u1 * scale, f32(0.0), ONE_MINUS_EPS)
        return some, p0, p1, pdf


# ---- SDTree + GuidingField (sdtree.rs, field.rs) ------------------------------------------------------------------------
DEFAULT_CONFIG = dict(train_iterations=4, guide_prob=0.5, spatial_c=4000.0, dtree_rho=0.01, dtree_max_depth=20, spatial_max_depth=24)


class Field:
    def __init__(self, bounds_min, bounds_max, cfg, h):
        self.cfg = dict(DEFAULT_CONFIG, **cfg)
        self.maps = Maps(h)
        lo, hi = np.asarray(bounds_min, f32), np.asarray(bounds_max, f32)
        pad = rmax(np.max(hi - lo) * f32(1e-3), f32(1e-3))  # field.rs:66
        self.bmin, self.bmax = (lo - pad).astype(f32), (hi + pad).astype(f32)
        self.nodes = [dict(leaf=True, dtree=0, sample_count=0)]
        self.dtrees = [DTree()]
        self.recorded = 0
        self._flat = None

    def flat(self):
        if self._flat is None:
            self._flat = Flat(self)
        return self._flat

    def leaf_index(self, pos):  # sdtree.rs:43-58, on the restatement's own nodes
        fl = self.flat()
        with np.errstate(invalid="ignore"):
            p = np.where(pos > self.bmin, pos, self.bmin)
            p = np.where(p < self.bmax, p, self.bmax).astype(f32)
            node = np.zeros(len(p), np.int64)
            while True:
                inner = fl.axis[node] != NO_CHILD
                if not inner.any():
                    return node
                ax = np.where(inner, fl.axis[node], 0)
                right = p[np.arange(len(p)), ax] >= fl.split[node]
                node = np.where(inner, np.where(right, fl.b[node], fl.a[node]), node)

    def update(self, samples, next_iteration):  # field.rs:101-112
        samples = np.asarray(samples, SAMPLE)
        if len(samples):
            p0, p1 = self.maps.dir_to_canonical(samples["dir"])
            leaf = self.leaf_index(samples["pos"])
            for l in np.unique(leaf):  # sdtree.rs:70-80: every sample counts, even if its flux is zero
                m = leaf == l
                self.nodes[l]["sample_count"] += int(m.sum())
                self.dtrees[self.nodes[l]["dtree"]].record(p0[m], p1[m], samples["radiance"][m])
            self.recorded += len(samples)
        self.refine(next_iteration)
        self._flat = None

    def refine(self, next_iteration):  # sdtree.rs:86-105
        c = self.cfg
        k = int(np.uint32(next_iteration).astype(np.int32))
        with np.errstate(all="ignore"):
            t = f64(f32(c["spatial_c"])) * np.sqrt(np.ldexp(f64(1.0), k))
        m = t if t > 1.0 else f64(1.0)  # f64::max(1.0)
        threshold = 2 ** 64 - 1 if m >= 2.0 ** 64 else int(m)  # `as u64` saturates
        self.split_rec(0, self.bmin.copy(), self.bmax.copy(), 0, threshold, c["spatial_max_depth"])
        rho = f32(c["dtree_rho"])
        self.dtrees = [d.refine(rho, c["dtree_max_depth"]) for d in self.dtrees]
        for n in self.nodes:
            if n["leaf"]:
                n["sample_count"] = 0

    def split_rec(self, node, lo, hi, depth, threshold, max_depth):  # sdtree.rs:107-168
        n = dict(self.nodes[node])
        if not n["leaf"]:
            max0, min1 = hi.copy(), lo.copy()
            max0[n["axis"]] = n["split"]; min1[n["axis"]] = n["split"]
            self.split_rec(n["children"][0], lo, max0, depth + 1, threshold, max_depth)
            self.split_rec(n["children"][1], min1, hi, depth + 1, threshold, max_depth)
            return
        if n["sample_count"] <= threshold or depth >= max_depth:
            return
        extent = hi - lo
        axis = 0 if (extent[0] >= extent[1] and extent[0] >= extent[2]) else (1 if extent[1] >= extent[2] else 2)
        split = f32(0.5) * (lo[axis] + hi[axis])
        dtree1 = len(self.dtrees)
        self.dtrees.append(self.dtrees[n["dtree"]].copy())
        c0 = len(self.nodes)
        self.nodes.append(dict(leaf=True, dtree=n["dtree"], sample_count=n["sample_count"] // 2))
        c1 = len(self.nodes)
        self.nodes.append(dict(leaf=True, dtree=dtree1, sample_count=n["sample_count"] // 2))
        self.nodes[node] = dict(leaf=False, axis=axis, split=split, children=(c0, c1))
        max0, min1 = hi.copy(), lo.copy()
        max0[axis] = split; min1[axis] = split
        self.split_rec(c0, lo, max0, depth + 1, threshold, max_depth)
        self.split_rec(c1, min1, hi, depth + 1, threshold, max_depth)

    def s_depth(self, node=0, depth=0):
        n = self.nodes[node]
        if n["leaf"]:
            return depth
        return max(self.s_depth(n["children"][0], depth + 1), self.s_depth(n["children"][1], depth + 1))

    def stats(self):
        return dict(s_nodes=len(self.nodes), s_leaves=sum(1 for n in self.nodes if n["leaf"]), s_depth=self.s_depth(),
                    d_trees=len(self.dtrees), d_nodes=sum(len(t.sums) for t in self.dtrees),
                    d_depth=max(t.depth() for t in self.dtrees), recorded=self.recorded)

    # GuidingField::sample / ::pdf (field.rs:88-97) as RESULT records, trained_at beside them
    def sample(self, q):
        q = np.asarray(q, QUERY)
        fl = self.flat()
        root = fl.dtree_at(q["pos"])
        some, p0, p1, pdf = fl.dtree_sample(root, np.ascontiguousarray(q["seed_u"]), np.ascontiguousarray(q["seed_v"]))
        out = np.zeros(len(q), RESULT)
        d = self.maps.canonical_to_dir(p0, p1)
        out["dir"] = np.where(some[:, None], d, f32(0.0))
        out["pdf"] = np.where(some, pdf, f32(0.0))
        out["some"] = some
        out["trained"] = DTree.total(fl.sums[root]) > 0
        return out

    def pdf(self, q):
        q = np.asarray(q, QUERY)
        fl = self.flat()
        root = fl.dtree_at(q["pos"])
        p0, p1 = self.maps.dir_to_canonical(q["dir"])
        out = np.zeros(len(q), RESULT)
        out["pdf"] = fl.dtree_pdf(root, p0, p1)
        out["some"] = 1
        out["trained"] = DTree.total(fl.sums[root]) > 0
        return out


def mismatches(got, want):
    """Records whose bits differ; a NaN on both sides counts as equal whatever its payload."""
    g = np.ascontiguousarray(got).view(u32).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(u32).reshape(len(want), -1)
    same = (g == w) | (np.isnan(g.view(f32)) & np.isnan(w.view(f32)))
    return np.nonzero(~same.all(axis=1))[0]
