"""No GPU: the one signature table of tf_kaldi_speaker_amd._lib against the prototypes of include/xvec_hip.h.  Every entry point
has the header's return type, argument count and, per argument, the header's scalar width or a pointer; the checker is then
run on doctored tables and has to name each doctored function.  The struct layouts and the XV_* constants are held to the
header by the compiled program of tests/test_host_logic.py."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import header_protos  # noqa: E402


@pytest.fixture(scope="module")
def bound(repo_root):
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    text = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    return _lib, text, header_protos.parse(text)


def test_the_parser_reads_every_declaration(bound):
    _lib, text, protos = bound
    assert set(protos) == header_protos.searched_names(text) and len(protos) >= 105
    assert protos["xv_version"] == ("const char*", [])
    assert protos["xv_create"] == ("int", ["const xv_model_desc*", "int", "xv_handle**"])
    assert protos["xv_pack_rows"] == ("int64_t", ["const void*const*", "const int64_t*", "int", "void*", "int"])
    assert protos["xv_plan_destroy"] == ("void", ["xv_plan*"]) and len(protos["xv_att_pool_backward"][1]) == 33


def test_every_entry_has_the_headers_signature(bound):
    _lib, _, protos = bound
    assert header_protos.check(_lib.SIGNATURES, protos, _lib) == []
    assert _lib.EXPORTS == [name for name, _, _ in _lib.SIGNATURES] == list(protos)         # the header's order
    lib = _lib.load()
    for name, restype, argtypes in _lib.SIGNATURES:                                         # and load() applies the table as it stands
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


def _edit(table, name, restype=None, argtypes=None):
    return [(n, restype(r) if n == name and restype else r, argtypes(list(a)) if n == name and argtypes else a) for n, r, a in table]


def _swapped(args):
    i = next(i for i in range(len(args) - 1) if args[i] is C.c_void_p and args[i + 1] is C.c_int64)
    return args[:i] + [args[i + 1], args[i]] + args[i + 2:]


def _narrowed(args):
    i = args.index(C.c_int64)
    return args[:i] + [C.c_int] + args[i + 1:]


MUTANTS = [
    ("xv_tconv_workspace", lambda t, L: _edit(t, "xv_tconv_workspace", restype=lambda r: C.c_int)),            # a restype narrowed
    ("xv_score_matrix", lambda t, L: _edit(t, "xv_score_matrix", argtypes=_narrowed)),                         # an int64 argument narrowed
    ("xv_att_pool_backward", lambda t, L: _edit(t, "xv_att_pool_backward", argtypes=lambda a: a[:20] + a[21:])),   # one argument dropped
    ("xv_forward", lambda t, L: _edit(t, "xv_forward", argtypes=_swapped)),                                    # a pointer and a scalar swapped
    ("xv_vbx", lambda t, L: [e for e in t if e[0] != "xv_vbx"]),                                               # one function removed
    ("xv_create", lambda t, L: _edit(t, "xv_create", argtypes=lambda a: [C.POINTER(L.PlanInfo)] + a[1:])),   # another struct
    ("xv_vad_energy", lambda t, L: _edit(t, "xv_vad_energy", argtypes=lambda a: [C.c_double if x is C.c_float else x for x in a])),
]


@pytest.mark.parametrize("name,doctor", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_checker_names_a_doctored_entry(bound, name, doctor):
    _lib, _, protos = bound
    problems = header_protos.check(doctor(list(_lib.SIGNATURES), _lib), protos, _lib)
    assert problems and {n for n, _ in problems} == {name}, problems


def test_workspace_sizes_beyond_32_bits_come_back_whole(bound):
    """The size queries are host code and answer without a device.  gz [total_out, round4(N)] floats alone is 2^32 - 2^19 bytes here."""
    lib = bound[0].load()
    total_out = (1 << 21) - 256
    for fn in (lib.xv_tconv_workspace, lib.xv_tconv_workspace_min):
        assert fn.restype is C.c_int64
        assert fn(64, 1 << 21, total_out, 5, 512, 512) >= 4 * total_out * 512 > 1 << 31
    assert lib.xv_tconv_forward_workspace.restype is C.c_int64
    # self-attentive pooling at the header's limits (batch 2^20, 2^24 rows, 16 heads, 4096 columns): gscore [total_rows, H] is
    # 2^30 bytes and the per-utterance planes of 2^20 utterances take both sizes far beyond 2^31 (826 GB and 276 GB)
    for fn in (lib.xv_att_pool_workspace, lib.xv_att_pool_workspace_min):
        assert fn.restype is C.c_int64
        assert fn(1 << 20, 1 << 24, 16, 4096, 4096, 0, 0) > 1 << 31
