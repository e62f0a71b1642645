"""The MFCC / VAD entry points are declared in include/xvec_hip.h, listed in _lib.EXPORTS and exported by the built library."""
import ctypes
import os
import re

NAMES = ["xv_mfcc_create", "xv_mfcc_destroy", "xv_mfcc_num_frames", "xv_mfcc_compute", "xv_vad_energy"]


def test_mfcc_symbols_are_declared_listed_and_exported(repo_root):
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    hdr = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    declared = set(re.findall(r"\b(xv_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    # the ctypes mirror has the size the header's struct has: 19 four-byte fields
    assert ctypes.sizeof(_lib.MfccOpts) == 19 * 4
    assert len(re.search(r"typedef struct \{([^}]*)\} xv_mfcc_opts;", hdr).group(1).strip().split(";")) - 1 == 19
    assert "mfcc.hip" in g.SOURCES and "mfcc.hip" not in g.AUDITED
