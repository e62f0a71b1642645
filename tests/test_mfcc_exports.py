"""The MFCC / VAD operator in the build recipe.  That its entry points are declared, listed and exported with the header's
signatures, and that xv_mfcc_opts has the header's layout, is tests/test_binding_host.py and tests/test_host_logic.py."""
import os
import re


def test_mfcc_symbols_are_declared_listed_and_exported(repo_root):
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    assert len(re.search(r"typedef struct \{([^}]*)\} xv_mfcc_opts;", hdr).group(1).strip().split(";")) - 1 == 19
    assert "mfcc.hip" in g.SOURCES and "mfcc.hip" not in g.AUDITED
