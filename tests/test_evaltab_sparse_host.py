"""CPU tier of abc_eval_tables_update_sparse: the symbol and its declaration, the untouched descriptor, and every refusal --
its own two and all of abc_eval_tables_update's -- each before any launch.  The dense entry point still accepts what it
accepted (a map whose h * w is no multiple of 32 included)."""
import ctypes as C
import os
import re

import pytest
import torch

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ["atom_mask", "bond_mask", "omega_mask", "rho_abs", "types", "charges", "hs", "t_atom", "t_types", "t_charges", "t_hs", "t_bond",
          "t_btypes", "t_rho", "t_omega"]
WORK = ["partial", "counts_last", "counts_totals", "meters_last", "meters_totals"]
FLAGS = 0x200000


def _desc():
    """a descriptor that would pass every check (the addresses are never dereferenced: each test breaks one field)"""
    d = L.EvalDesc()
    for i, f in enumerate(INPUTS + WORK + ["btypes"]):
        setattr(d, f, 0x1000 * (i + 1))
    d.B, d.h, d.w = 2, 32, 32
    return d


def _refused(d, flags, word):
    lib = L.load()
    assert lib.abc_eval_tables_update_sparse(C.byref(d), flags, None) == -1          # ABC_EINVAL, before any launch
    assert word in lib.abc_last_error().decode(), lib.abc_last_error()


def test_symbol_is_exported_and_declared():
    lib = L.load()
    assert "abc_eval_tables_update_sparse" in L.SYMBOLS
    assert lib.abc_eval_tables_update_sparse.argtypes is not None and len(lib.abc_eval_tables_update_sparse.argtypes) == 3
    with open(os.path.join(ROOT, "include", "abcnet_hip.h")) as f:
        text = f.read()
    assert re.search(r"int\s+abc_eval_tables_update_sparse\(const abc_eval_desc\*\s*d,\s*const uint32_t\*\s*target_flags,\s*abc_stream_t\s+stream\);", text)
    assert re.search(r"int\s+abc_eval_tables_update\(const abc_eval_desc\*\s*d,\s*abc_stream_t\s+stream\);", text)


def test_descriptor_is_unchanged():
    lib = L.load()
    assert lib.abc_eval_desc_size() == C.sizeof(L.EvalDesc)
    # 17 input pointers, n_valid, three int32 (padded to 16 bytes), five workspace pointers: the layout the dense entry point shipped with
    assert C.sizeof(L.EvalDesc) == 18 * 8 + 16 + 5 * 8
    assert L.EvalDesc not in L._STRUCTS


def test_null_flags_are_refused():
    _refused(_desc(), None, "target_flags")


@pytest.mark.parametrize("B,h,w", [(3, 5, 5), (2, 40, 30), (1, 1, 16), (2, 33, 16)])
def test_pixel_count_no_multiple_of_32_is_refused(B, h, w):
    d = _desc()
    d.B, d.h, d.w = B, h, w
    assert (h * w) % 32
    _refused(d, FLAGS, "multiple of 32")
    # (the dense entry point counts blocks for such a shape as before)
    assert L.load().abc_eval_tables_blocks(C.byref(d)) == (B * h * w + 255) // 256


@pytest.mark.parametrize("field", ["B", "h", "w"])
def test_empty_shape_is_refused(field):
    d = _desc()
    setattr(d, field, 0)
    _refused(d, FLAGS, "empty")


def test_oversized_shape_is_refused():
    d = _desc()
    d.B, d.h, d.w = 4, 32768, 32768
    _refused(d, FLAGS, "2^31")


@pytest.mark.parametrize("field", WORK)
def test_null_workspace_is_refused(field):
    d = _desc()
    setattr(d, field, None)
    _refused(d, FLAGS, "workspace")


@pytest.mark.parametrize("field", INPUTS)
def test_null_input_is_refused(field):
    d = _desc()
    setattr(d, field, None)
    _refused(d, FLAGS, "null")


def test_bond_type_source_must_be_exactly_one():
    d = _desc()
    d.btype_idx = 0x100000
    _refused(d, FLAGS, "exactly one")
    d.btypes, d.btype_idx = None, None
    _refused(d, FLAGS, "exactly one")


def test_dense_entry_point_has_no_new_refusal():
    """a shape the sparse form refuses passes every check of abc_eval_tables_update up to its LAST one (both bond-type sources
    set), whose text is the old one; with one source the call is accepted: without a device the launch itself is what fails
    (ABC_ELAUNCH), with one tests/test_gpu_evaltab_sparse.py runs this shape on real tensors"""
    lib = L.load()
    d = _desc()
    d.B, d.h, d.w = 3, 5, 5
    d.btype_idx = 0x100000
    assert lib.abc_eval_tables_update(C.byref(d), None) == -1
    assert "exactly one" in lib.abc_last_error().decode()
    d.btype_idx = None
    if not torch.cuda.is_available():
        assert lib.abc_eval_tables_update(C.byref(d), None) == -3, lib.abc_last_error()
        d.B, d.h, d.w = 2, 32, 32
        assert lib.abc_eval_tables_update_sparse(C.byref(d), FLAGS, None) == -3, lib.abc_last_error()
