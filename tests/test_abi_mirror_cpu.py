"""One header of include/ <-> one table of `_lib.HEADERS` <-> one op module, checked for every header and every pair of headers
(no compute on a GPU).  A wrong entry in a ctypes table is not an exception but a launch with garbage arguments, so each table is
compared with its header declaration by declaration: argument count, and the kind of every argument and of the return value."""
import ctypes
import itertools
import os

import pytest
import torch

import abi

HEADERS = list(abi.OP_MODULES)


def test_every_header_has_a_table_and_an_op_module():
    from cvpce_amd import _lib
    on_disk = sorted(f for f in os.listdir(abi.INCLUDE) if f.endswith('.h'))
    assert on_disk == sorted(_lib.HEADERS) == sorted(abi.OP_MODULES)
    assert sorted(abi.PINNED_NAMES) == sorted(abi.FEATURES) and set(abi.FAMILY_WORDS) == set(abi.FEATURES) - {'cvpce_amd_gaussians.h'}
    assert _lib.HEADERS[abi.INFERENCE] is _lib.SIGNATURES
    entry_points = sum(len(table) for table in _lib.HEADERS.values())
    ops = sum(len(abi.op_module(h).NAMES) for h in HEADERS)
    print(f'{len(on_disk)} headers, {entry_points} entry points, {ops} ops')
    assert (len(on_disk), entry_points, ops) == (14, 88, 59)
    declared = {s for h in HEADERS for s in abi.header_symbols(h)}
    assert abi.HOST_ONLY <= declared and {s for s in declared if s.endswith('_bytes')} <= abi.HOST_ONLY and len(abi.HOST_ONLY) == 12


@pytest.mark.parametrize('header', HEADERS)
def test_header_table_and_library_agree(header):
    from cvpce_amd import _lib
    table, symbols = _lib.HEADERS[header], abi.header_symbols(header)
    assert sorted(table) == symbols, f'ctypes signature table out of sync with include/{header}'
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for fn in symbols:
        assert hasattr(exported, fn), f'{fn} declared in include/{header} but not exported'
        assert getattr(_lib.lib, fn).restype == table[fn][0] and getattr(_lib.lib, fn).argtypes == table[fn][1], f'{fn}: the table is not bound'


@pytest.mark.parametrize('header', HEADERS)
def test_declarations_and_ctypes_agree_in_count_and_kind(header):
    from cvpce_amd import _lib
    table, declared = _lib.HEADERS[header], abi.declarations(header)
    assert sorted(declared) == abi.header_symbols(header), 'a declaration the parser cannot read'
    for fn, (c_ret, c_args) in declared.items():
        restype, argtypes = table[fn]
        assert len(argtypes) == len(c_args), f'{fn}: {len(c_args)} arguments declared, {len(argtypes)} in the table'
        assert abi.ctypes_kind(restype) == c_ret, f'{fn}: returns {c_ret}, the table says {abi.ctypes_kind(restype)}'
        for i, (t, kind) in enumerate(zip(argtypes, c_args)):
            assert abi.ctypes_kind(t) == kind, f'{fn}: argument {i} is declared {kind}, the table says {abi.ctypes_kind(t)}'


def test_headers_and_tables_are_pairwise_disjoint():
    from cvpce_amd import _lib
    for a, b in itertools.combinations(HEADERS, 2):
        assert not set(abi.header_symbols(a)) & set(abi.header_symbols(b)), (a, b)
        assert not set(_lib.HEADERS[a]) & set(_lib.HEADERS[b]), (a, b)


def test_a_family_word_stays_in_its_family():
    from cvpce_amd import _lib
    found = set()
    for header, word in abi.FAMILY_WORDS.items():
        for other in HEADERS:
            if other != header:
                names = set(abi.header_symbols(other)) | set(_lib.HEADERS[other]) | {'cvpce_' + n for n in abi.op_module(other).NAMES}
                found |= {(word, n) for n in names if word in n}
    assert found == abi.FAMILY_EXCEPTIONS


@pytest.mark.parametrize('header', abi.FEATURES)
def test_feature_ops_are_the_header_s_launches(header):
    names = abi.op_module(header).NAMES
    assert names == abi.PINNED_NAMES[header]
    assert sorted('cvpce_' + n for n in names) == abi.op_symbols(header)


def test_inference_ops_cover_the_inference_header():
    """One op per compute entry point of include/cvpce_amd.h.  The fp16 twins of the detector's kernels are reached through the SAME
    ops: the op picks the entry point by the activations' dtype (torch_ops._by_dtype) -- every twin has its bf16 original declared.
    (The two 3x3 halo entry points share one op: Cout <= 128 is forwarded to the wide-tile kernel inside the library; atlas_copy has
    two ops.)"""
    from cvpce_amd import torch_ops
    symbols = set(abi.header_symbols(abi.INFERENCE))
    assert len(symbols) >= 13
    f16 = {s for s in symbols if s.endswith('_f16')}
    assert len(f16) == 16 and f16 == abi.twins(symbols)
    assert len(torch_ops.NAMES) == len(abi.op_symbols(abi.INFERENCE)) == 37


def test_op_names_are_distinct_and_gpu_only():
    names = [n for h in HEADERS for n in abi.op_module(h).NAMES]
    assert len(names) == len(set(names)) == 59
    for name in names:
        assert hasattr(torch.ops.cvpce_amd, name)
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'cvpce_amd::{name}', 'CUDA'), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'cvpce_amd::{name}', 'CPU'), name
