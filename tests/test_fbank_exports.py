"""The fbank operator in the build recipe and the field order of its options.  That its entry points are declared, listed and
exported with the header's signatures is tests/test_binding_host.py."""
import ctypes
import os
import re


def test_fbank_symbols_are_declared_listed_and_exported(repo_root):
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    hdr = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    # the ctypes mirror has the size and the field order the header's struct has
    body = re.search(r"typedef struct \{([^}]*)\} xv_fbank_opts;", hdr).group(1)
    fields = re.findall(r"^\s*(?:int32_t|float)\s+(\w+);", body, flags=re.M)
    assert len(body.strip().split(";")) - 1 == len(fields) == 19
    assert ctypes.sizeof(_lib.FbankOpts) == len(fields) * 4
    assert [f for f, _ in _lib.FbankOpts._fields_] == fields
    for (f, t), c in zip(_lib.FbankOpts._fields_, re.findall(r"^\s*(int32_t|float)\s+\w+;", body, flags=re.M)):
        assert t is (ctypes.c_int32 if c == "int32_t" else ctypes.c_float), f
    # the kernel lives in the MFCC's translation unit: no new source in the build recipe
    assert "fbank_kernel" in open(os.path.join(g.CSRC, "mfcc.hip")).read() and not any("fbank" in s for s in g.SOURCES)
