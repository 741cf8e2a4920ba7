"""The per-pixel camera table and the sample cursor (kernels/camera_pixel.hip.h: pixel_record, what k_fill_pixel_table
runs per owned pixel; sample_cursor / sample_cursor_next, what the camera launches step instead of dividing) WITHOUT a GPU:
the header compiled as host C++ (tests/host_shade/pixel_table_host.cpp).

The table: every one of a record's eight words equals what camera_sample's computed form works out for that pixel — restated
call for call from the sampler's functions — and what the oracle's sampler (oracle/ora_qmc.h) gives; a draw off the stored
seeds equals draw_sample4 on the K_CAMERA domain and the oracle's draw, bit for bit. Over a 64 x 32 frame dealt to three
ranks: the shards of rank 0 (three tiles) and rank 2 (two tiles), as the library deals them.

The cursor: (pix, sl) equal (g % n_act, g / n_act) at every round, for n_act in {1, 255, 256, 257, 20 736} x grids of
{1, 3, 2048} workgroups x 40 rounds, and for sample numbers above 2^32.

The same file is built once more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_shade", "pixel_table_host.cpp")
FLAGS = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
         "-I" + os.path.join(ROOT, "profiles", "host_shade"), "-I" + os.path.join(ROOT, "crust-render_amd", "csrc", "kernels"),
         "-I" + os.path.join(ROOT, "oracle")]
W, H, WORLD = 64, 32, 3
BLOCK = 256


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("pixel_table_host") / "libpixel_table_host.so"
    res = subprocess.run(FLAGS + ["-fPIC", "-shared", SRC, "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    L = C.CDLL(str(out))
    up = C.POINTER(C.c_uint32)
    L.pixel_table_fill.argtypes = [up, C.c_size_t, C.c_uint32, C.c_int, up]
    L.pixel_table_fill.restype = None
    L.pixel_table_computed.argtypes = [up, C.c_size_t, C.c_uint32, C.c_int, C.c_int, up, up]
    L.pixel_table_computed.restype = None
    L.pixel_table_draw_mismatches.argtypes = [up, C.c_size_t, C.c_uint32, C.c_int, up, C.c_size_t]
    L.pixel_table_draw_mismatches.restype = C.c_size_t
    L.sample_cursor_mismatches.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_uint32, C.c_uint32]
    L.sample_cursor_mismatches.restype = C.c_size_t
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


@pytest.fixture(scope="module")
def shards(crt):
    out = [np.ascontiguousarray(crt.shard.shard_pixels(W, H, rank, WORLD), np.uint32) for rank in (0, 2)]
    assert len(out[0]) == 3 * 256 and len(out[1]) == 2 * 256  # two shards of different size
    return out


@pytest.mark.parametrize("frame", [0, 7, -3])
def test_every_record_word_is_the_computed_forms(host, shards, frame):
    for pix in shards:
        n = len(pix)
        table = np.zeros((n, 8), np.uint32)
        host.pixel_table_fill(_p(pix), n, W, frame, _p(table))
        for index in (0, 11):  # the sample index reaches no word of the record
            computed, oracle = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
            host.pixel_table_computed(_p(pix), n, W, frame, index, _p(computed), _p(oracle))
            assert np.array_equal(table, computed)
            assert np.array_equal(table, oracle)
        # px, py: the floats of the pixel's coordinates, in the list's order
        assert np.array_equal(table[:, 0].view(np.float32), (pix % W).astype(np.float32))
        assert np.array_equal(table[:, 1].view(np.float32), (pix // W).astype(np.float32))
        assert len(np.unique(table[:, 7])) == n  # a pattern per pixel, not one for all


def test_draws_off_the_stored_seeds_are_the_samplers(host, shards):
    idx = np.array([0, 1, 2, 7, 255, 256, 511, 65535, 0x12345678], np.uint32)
    for pix in shards:
        assert host.pixel_table_draw_mismatches(_p(pix), len(pix), W, 3, _p(idx), len(idx)) == 0


def test_cursor_sweep(host):
    """Every lane class of a workgroup (first, last lane), first and last workgroup of the grid."""
    for n_act in (1, 255, 256, 257, 20736):
        for grid in (1, 3, 2048):
            step = grid * BLOCK
            for block in {0, grid - 1}:
                for lane in (0, 63, 255):
                    g0 = block * BLOCK + lane
                    assert host.sample_cursor_mismatches(g0, step, n_act, 40) == 0, (n_act, grid, block, lane)


def test_cursor_above_two_to_the_32(host):
    assert host.sample_cursor_mismatches((1 << 32) + 12345, 2048 * BLOCK, 4_000_000_000, 40) == 0
    assert host.sample_cursor_mismatches((1 << 40) + 99, 16384 * BLOCK, 1920 * 1080, 40) == 0
    # and a wrong cursor is seen: a step the cursor was not built for
    assert host.sample_cursor_mismatches(5, 0, 7, 3) == 0  # step 0 stays put
    assert host.sample_cursor_mismatches(0, (1 << 32) + 1, 0xFFFFFFFF, 40) == 0


def test_stand_alone_under_sanitizers(tmp_path):
    exe = tmp_path / "pixel_table_san"
    res = subprocess.run(FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPIXEL_TABLE_MAIN", SRC, "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "0 mismatches" in run.stdout
