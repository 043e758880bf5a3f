"""CPU part of the size-selected-form tests, on host-only handles: the info calls that report a launch's form
against hand arithmetic on both sides of every threshold, the batch sizes tests/size_forms.py chooses, and the block-wise checker
with its teeth on small arrays (and on one array whose flat index passes 2^31)."""
import os
import re

import numpy as np
import pytest

import size_forms as SF
from conftest import ROOT

RECORD_PROBLEM = "stress-12x100"     # part A of its records has 500 nodes: not a multiple of 64, so the flat mapping and the runs apply


def _aero(name):
    E, _prob, _x0 = SF.engine(name, 0, "aero_all", device=-1)
    return E


@pytest.mark.parametrize("name,nodes", [("mixed-6x64", 325), ("stress-12x128", 1419)])
def test_dense_aero_launch_info_against_hand_arithmetic(name, nodes):
    """gel_eval_aero_all_device's arrays: flat while the largest kind's gradient values stay below 2^32 - 2^24 bytes, one tile per
    vector from there on and for one vector; never in runs"""
    E = _aero(name)
    assert [E.aero_dims(k)[0] for k in E.AERO_KINDS] == [nodes] * 3 and nodes >= 64 and nodes % 64 != 0
    per = 12 * nodes * 8                                         # alpha / q-alpha: [R][8 + 4] doubles
    assert SF.aero_dense_bytes(E) == per
    last_flat = ((1 << 32) - (1 << 24) - 1) // per
    for B, flat in ((1, 0), (2, 1), (256, 1), (last_flat, 1), (last_flat + 1, 0), (4 * last_flat, 0)):
        assert E.aero_launch_info(B) == {"flat": flat, "runs": 1, "run_len": B, "max_bytes": B * per}, B
    # what the helper chooses crosses what it claims
    Bn, Bt = SF.aero_dense_B(E, "negative"), SF.aero_dense_B(E, "tiles")
    assert Bn % SF.P == 0 and Bt % SF.P == 0 and Bn < Bt
    assert (Bn - SF.P) * per <= 2 ** 31 < Bn * per and E.aero_launch_info(Bn)["flat"] == 1
    assert E.aero_launch_info(Bt)["flat"] == 0 and E.aero_launch_info(Bt - SF.P)["flat"] == 1
    assert Bt - SF.P <= last_flat < Bt


def test_record_aero_launch_info_against_hand_arithmetic():
    """part A of gel_eval_batch_aero_device's records where aero_kernel writes it: runs of (2^32 - 2^25) / (8 width) vectors, each
    flat (a run of one vector: a tile).  At mixed-6x64 and stress-12x128 part A has 5 x 64 and 5 x 128 nodes -- multiples of 64, whole
    tiles -- so those take one tile per vector with 64-bit addresses at every B and are never split."""
    for name, nodes in (("mixed-6x64", 320), ("stress-12x128", 640)):
        E = _aero(name)
        width = E.aero_record_layout()[0]
        assert nodes % 64 == 0
        for B in (1, 256, 65536, 1 << 20):
            assert E.aero_launch_info(B, records=True) == {"flat": 0, "runs": 1, "run_len": B, "max_bytes": B * width * 8}, (name, B)
    E = _aero(RECORD_PROBLEM)
    width = E.aero_record_layout()[0]
    run = ((1 << 32) - (1 << 25)) // (8 * width)
    assert run * width * 8 > 2 ** 31                             # a full run reaches the offsets that are negative as int
    for B, runs in ((1, 1), (2, 1), (run, 1), (run + 1, 2), (2 * run, 2), (2 * run + 1, 3)):
        info = E.aero_launch_info(B, records=True)
        rl = run if runs > 1 else B
        assert info == {"flat": int(rl > 1), "runs": runs, "run_len": rl, "max_bytes": rl * width * 8}, (B, info)
    # the dense arrays of the same handle are not split
    assert E.aero_launch_info(4 * run)["runs"] == 1


def test_aero_launch_info_without_rows_and_argument_errors():
    import ctypes as C
    from gelato_amd import _lib
    E, _p, _x = SF.engine("mixed-6x64", device=-1)
    assert E.aero_launch_info(70000) == {"flat": 0, "runs": 1, "run_len": 70000, "max_bytes": 0}
    L = _lib.lib()
    info = (C.c_int64 * 4)()
    assert L.gel_aero_launch_info(E._h, 0, 0, info) == -1 and L.gel_aero_launch_info(None, 1, 0, info) == -1
    assert L.gel_aero_launch_info(E._h, 1, 0, None) == -1 and L.gel_jac_products_launch_info(E._h, None) == -1
    assert L.gel_jac_products_launch_info(None, (C.c_int32 * 4)()) == -1


def _lds_fit(nin, vb, transpose):
    return 8 * (nin * vb + (8 * vb if transpose else 0)) <= 64 * 1024      # gel_jprod.h jprod_lds_bytes / kJprodMaxLds


@pytest.mark.parametrize("name", ["example", "mixed-6x64", "stress-12x128", "ragged"])
def test_products_launch_info_honours_the_switches(name, monkeypatch):
    """VB: the largest of 8, 4, 2, 1 whose staged inputs fit 64 KB, or GEL_JPROD_VB where that fits (read per call); lanes per
    workgroup: 512, or GEL_JPROD_THREADS = 256 (read when the handle is created) -- as jprod_device launches"""
    monkeypatch.delenv("GEL_JPROD_VB", raising=False)
    monkeypatch.delenv("GEL_JPROD_THREADS", raising=False)
    E, _p, _x = SF.engine(name, device=-1)
    nn = [int(n) for n in E.num_nodes]
    # a phase's slice of the input: J v reads its state nodes (11 per node, n + 1 nodes), controls (2 n) and both knot times;
    # J^T lambda reads its 11 n residual rows
    nin = (max(11 * (n + 1) + 2 * n + 2 for n in nn), max(11 * n for n in nn))
    default = [max(vb for vb in (1, 2, 4, 8) if _lds_fit(nin[t], vb, t)) for t in (0, 1)]
    info = E.jac_products_info()
    assert [info["vb"], info["vb_t"]] == default and info["threads"] == info["threads_t"] == 512
    for vb in (1, 2, 4, 8):
        monkeypatch.setenv("GEL_JPROD_VB", str(vb))
        info = E.jac_products_info()
        assert [info["vb"], info["vb_t"]] == [vb if _lds_fit(nin[t], vb, t) else default[t] for t in (0, 1)], vb
    for bad in ("3", "16", "0", "x"):
        monkeypatch.setenv("GEL_JPROD_VB", bad)
        info = E.jac_products_info()
        assert [info["vb"], info["vb_t"]] == default
    monkeypatch.delenv("GEL_JPROD_VB")
    for env, want in (("256", 256), ("512", 512), ("128", 512)):
        monkeypatch.setenv("GEL_JPROD_THREADS", env)
        E2, _p, _x = SF.engine(name, device=-1)
        info = E2.jac_products_info()
        assert info["threads"] == info["threads_t"] == want and [info["vb"], info["vb_t"]] == default
    assert E.jac_products_info()["threads"] == 512                # read when the handle was created


def test_mesh_vectors_per_workgroup_constant():
    """test_size_forms.py derives mesh_kernel's vectors per workgroup as 512 // (n + 1): the workgroup size it divides"""
    text = open(os.path.join(ROOT, "gelato_amd", "csrc", "gel_mesh.h")).read()
    assert re.search(r"constexpr\s+int\s+kMeshMaxThreads\s*=\s*512\s*;", text)
    text = open(os.path.join(ROOT, "gelato_amd", "csrc", "gel_host.hip")).read()
    assert re.search(r"q\.vpb\s*=\s*gel::kMeshMaxThreads\s*/\s*P\s*;", text)


def test_mesh_vectors_per_workgroup_where_the_lds_binds():
    """... unless 64 KB of LDS hold fewer beside the tables (gel_mesh.h mesh_vectors_per_group, reported by gel_table_limits): not at
    the phases test_size_forms.py uses, 167 instead of 170 at n = 2 with the example's tables, 149 with 160 wind and 48 CA rows"""
    from gelato_amd import _lib
    for name, n in (("mixed-6x64", 64), ("stress-12x128", 128)):
        E, prob, _x = SF.engine(name, device=-1)
        assert n in [int(v) for v in E.num_nodes]
        assert _lib.table_limits(len(prob["wind_table"]), len(prob["ca_table"]), n)["mesh_vectors"] == 512 // (n + 1), name
    assert _lib.table_limits(7, 9, 2)["mesh_vectors"] == (8192 - 148) // 48 == 167 < 512 // 3
    assert _lib.table_limits(160, 48, 2)["mesh_vectors"] == (8192 - 1030) // 48 == 149
    assert _lib.table_limits(320, 32, 500)["mesh_vectors"] == 1 and _lib.table_limits(7, 9, 512)["mesh_vectors"] == -1


def test_batch_size_helpers():
    assert SF.round_up(1) == 256 and SF.round_up(256) == 256 and SF.round_up(257) == 512
    assert SF.first_multiple_past(2 ** 31, 607424) == 3584 and 3584 * 607424 > 2 ** 31 >= 3328 * 607424
    assert SF.first_multiple_past(1024, 4, m=256) == 512          # 256 vectors hold exactly the threshold: not past it
    assert SF.first_multiple_where(lambda B: B >= 1000, 256, 4096) == 1024
    assert SF.first_multiple_where(lambda B: B > 256, 256, 512) == 512
    with pytest.raises(AssertionError):
        SF.first_multiple_where(lambda B: True, 256, 512)


# ---- the checker --------------------------------------------------------------------------------------------------------------
def _tiled(ref, B):
    return np.ascontiguousarray(np.tile(ref, (-(-B // len(ref)), 1))[:B])


@pytest.mark.parametrize("B", [256, 512, 1000, 255, 1])
@pytest.mark.parametrize("chunk", [SF.CHUNK_ELEMS, 256 * 7, 1])
def test_checker_passes_and_finds_every_planted_bit(B, chunk):
    rng = np.random.default_rng(B)
    ref = rng.standard_normal((SF.P, 7))
    ref[3, 2], ref[4, 2], ref[5, 5] = np.nan, -0.0, np.inf
    out = _tiled(ref, B)
    assert SF.first_mismatch(out, ref, chunk_elems=chunk) is None
    for row, cell, bit in ((0, 0, 0), (B - 1, 6, 0), (B // 2, 3, 63), (B - 1, 0, 52)):
        SF.flip_bit(out, row, cell, bit)
        assert SF.first_mismatch(out, ref, chunk_elems=chunk) == (row, cell)
        SF.flip_bit(out, row, cell, bit)
    assert SF.first_mismatch(out, ref, chunk_elems=chunk) is None
    # the first difference in row-major order is the one reported
    if B > 2:
        SF.flip_bit(out, B - 1, 1)
        SF.flip_bit(out, 1, 4)
        assert SF.first_mismatch(out, ref, chunk_elems=chunk) == (1, 4)


def test_checker_compares_bits_not_values():
    ref = np.zeros((SF.P, 2))
    out = _tiled(ref, 512)
    out[300, 1] = -0.0                                           # equal as a value
    assert SF.first_mismatch(out, ref) == (300, 1)
    ref[:] = np.nan
    out = _tiled(ref, 512)
    assert SF.first_mismatch(out, ref) is None                   # the same NaN is the same bits
    SF.flip_bit(out, 511, 0, 3)                                  # another NaN
    assert np.isnan(out[511, 0]) and SF.first_mismatch(out, ref) == (511, 0)


def test_checker_with_selected_cells():
    import torch
    rng = np.random.default_rng(1)
    ref = rng.standard_normal((SF.P, 9))
    out = _tiled(ref, 700)
    cols = torch.tensor([1, 2, 5, 8])
    out[:, [0, 3, 4, 6, 7]] = 7.0                                # cells nobody names may hold anything
    assert SF.first_mismatch(out, ref) == (0, 0) and SF.first_mismatch(out, ref, cols) is None
    SF.flip_bit(out, 699, 5)
    assert SF.first_mismatch(out, ref, cols) == (699, 5)
    SF.flip_bit(out, 699, 5)
    shown = SF.check_blocks(out, ref, "selected", rows=(256,), cols=cols)
    assert (699, 8) in shown and all(c in (1, 2, 5, 8) for _r, c in shown)


def test_check_blocks_shows_its_teeth_and_restores():
    rng = np.random.default_rng(2)
    ref = rng.standard_normal((SF.P, 5))
    out = _tiled(ref, 1030)
    keep = out.copy()
    shown = SF.check_blocks(out, ref, "small", rows=(515,))
    assert shown == [(1029, 4), (515, 0)] and np.array_equal(out.view(np.int64), keep.view(np.int64))
    out[700, 2] += 1.0
    with pytest.raises(AssertionError, match="row 700 .vector 188 of the 256 distinct ones., cell 2"):
        SF.check_blocks(out, ref, "small")


def test_teeth_cells_past_the_thresholds():
    w = 607424
    assert SF.teeth_cells(3584, w) == [(3583, w - 1), divmod(2 ** 28, w), divmod(2 ** 31, w)]
    assert SF.teeth_cells(1024, w) == [(1023, w - 1), divmod(2 ** 28, w)]       # 2^31 bytes passed, 2^31 elements not
    assert SF.teeth_cells(256, 100) == [(255, 99)]
    assert SF.teeth_cells(256, 100, rows=(7,)) == [(255, 99), (7, 0)]


def test_checker_past_two_to_the_31_elements():
    """a flat index beyond 2^31 (one byte per element: 2.1 GB of host memory; the device tests do the same with doubles)"""
    import torch
    w = 4096
    B = 2 ** 31 // w + 2 * SF.P
    ref = (torch.arange(SF.P * w, dtype=torch.int64) % 251).to(torch.int8).reshape(SF.P, w)
    out = ref.repeat(B // SF.P, 1)
    assert out.numel() > 2 ** 31 and out.is_contiguous()
    cells = SF.teeth_cells(B, w, itemsize=1)
    assert cells == [(B - 1, w - 1), (2 ** 31 // w, 0)]          # 2^31 bytes = 2^31 elements here
    assert SF.check_blocks(out, ref, "int8") == cells
    SF.flip_bit(out, 2 ** 31 // w, 1)
    assert SF.first_mismatch(out, ref) == (2 ** 31 // w, 1)
