"""Host: tools/isa_same.py, the kernel-by-kernel comparison of two device-assembly files that decides whether a refactor of
a hand-scheduled unit changed any kernel.  Two tiny hand-written files in the layout hipcc -S --cuda-device-only emits."""
import importlib.util
import os

import pytest


def _kernel(name, body):
    return """\t.protected\t%(n)s ; -- Begin function %(n)s
\t.globl\t%(n)s
\t.type\t%(n)s,@function
%(n)s:                                  ; @%(n)s
; %%bb.0:
%(b)s\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(n)s
\t\t.amdhsa_next_free_vgpr 8
\t.end_amdhsa_kernel
\t.text
.Lfunc_end_%(n)s:
\t.size\t%(n)s, .Lfunc_end_%(n)s-%(n)s
                                        ; -- End function
; NumVgprs: 8
""" % {"n": name, "b": body}


def _file(kernels, cuid):
    return ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.text\n" + "".join(_kernel(n, b) for n, b in kernels)
            + "\t.type\t__hip_cuid_%(c)s,@object\n__hip_cuid_%(c)s:\n\t.byte\t0\n\t.amdgpu_metadata\n---\namdhsa.kernels: []\n...\n"
            "\t.end_amdgpu_metadata\n" % {"c": cuid})


A = ("_Z6kern_aPf", "\tv_mov_b32_e32 v1, 0\n\tglobal_store_dword v0, v1, s[0:1]\n")
B = ("_Z6kern_bPf", "\tv_add_f32_e32 v1, v1, v2\n\tglobal_store_dword v0, v1, s[0:1]\n")


@pytest.fixture(scope="module")
def isa_same(repo_root):
    spec = importlib.util.spec_from_file_location("isa_same", os.path.join(repo_root, "tools", "isa_same.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(isa_same, tmp_path, capsys, old, new):
    (tmp_path / "old.s").write_text(old)
    (tmp_path / "new.s").write_text(new)
    rc = isa_same.main(["isa_same.py", str(tmp_path / "old.s"), str(tmp_path / "new.s")])
    return rc, capsys.readouterr().out


def test_identical_files_but_for_the_cuid_hash_are_the_same(isa_same, tmp_path, capsys):
    rc, out = _run(isa_same, tmp_path, capsys, _file([A, B], "0123456789abcdef"), _file([A, B], "fedcba9876543210"))
    assert rc == 0 and out.strip() == "same: 2 kernels"


def test_one_changed_instruction_names_its_kernel_only(isa_same, tmp_path, capsys):
    b2 = (B[0], B[1].replace("v_add_f32_e32 v1, v1, v2", "v_add_f32_e32 v1, v1, v3"))
    rc, out = _run(isa_same, tmp_path, capsys, _file([A, B], "00"), _file([A, b2], "11"))
    assert rc == 1
    assert out.splitlines() == ["differs  _Z6kern_bPf (17 -> 17 lines, first at line 6 of the kernel)"]


def test_a_missing_kernel_is_reported_as_removed_and_a_new_one_as_added(isa_same, tmp_path, capsys):
    rc, out = _run(isa_same, tmp_path, capsys, _file([A, B], "00"), _file([A], "00"))
    assert rc == 1 and out.splitlines() == ["removed  _Z6kern_bPf"]
    rc, out = _run(isa_same, tmp_path, capsys, _file([A], "00"), _file([A, B], "00"))
    assert rc == 1 and out.splitlines() == ["added    _Z6kern_bPf"]


# ---- second verdict: "same up to commuted multiplicands"
PK = "\tv_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]\n\tglobal_store_dwordx2 v0, v[2:3], s[0:1]\n"


def _pk(isa_same, tmp_path, capsys, old_line, new_line, *flags):
    old, new = ("_Z6kern_cPf", PK), ("_Z6kern_cPf", PK.replace(old_line, new_line))
    assert old[1] != new[1]
    (tmp_path / "old.s").write_text(_file([A, old], "00"))
    (tmp_path / "new.s").write_text(_file([A, new], "11"))
    rc = isa_same.main(["isa_same.py", *flags, str(tmp_path / "old.s"), str(tmp_path / "new.s")])
    return rc, capsys.readouterr().out.splitlines()


def test_swapped_multiplicands_with_their_op_sel_hi_bits_are_commuted(isa_same, tmp_path, capsys):
    swap = ("v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]", "v[6:7], v[4:5], v[8:9] op_sel_hi:[0,1,1]")
    rc, out = _pk(isa_same, tmp_path, capsys, *swap)
    assert rc == 1 and out == ["commuted _Z6kern_cPf (1 lines)"]
    rc, out = _pk(isa_same, tmp_path, capsys, *swap, "--allow-commuted")
    assert rc == 0 and out == ["commuted _Z6kern_cPf (1 lines)"]


def test_an_array_that_becomes_all_default_after_the_swap_is_still_commuted(isa_same, tmp_path, capsys):
    rc, out = _pk(isa_same, tmp_path, capsys, "v_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]",
                  "v_pk_fma_f32 v[2:3], v[6:7], v[4:5], v[8:9] op_sel_hi:[0,1,1] neg_lo:[0,0,0]", "--allow-commuted")
    assert rc == 0 and out == ["commuted _Z6kern_cPf (1 lines)"]


def test_swapped_multiplicands_without_the_permuted_modifier_differ(isa_same, tmp_path, capsys):
    rc, out = _pk(isa_same, tmp_path, capsys, "v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]", "v[6:7], v[4:5], v[8:9] op_sel_hi:[1,0,1]",
                  "--allow-commuted")
    assert rc == 1 and out == ["differs  _Z6kern_cPf (17 -> 17 lines, first at line 6 of the kernel)"]


def test_a_swapped_subtraction_differs(isa_same, tmp_path, capsys):
    old, new = "\tv_sub_f32_e32 v2, v4, v6\n", "\tv_sub_f32_e32 v2, v6, v4\n"
    (tmp_path / "old.s").write_text(_file([("_Z6kern_dPf", old)], "00"))
    (tmp_path / "new.s").write_text(_file([("_Z6kern_dPf", new)], "00"))
    rc = isa_same.main(["isa_same.py", "--allow-commuted", str(tmp_path / "old.s"), str(tmp_path / "new.s")])
    assert rc == 1 and capsys.readouterr().out.splitlines() == ["differs  _Z6kern_dPf (16 -> 16 lines, first at line 6 of the kernel)"]


def test_a_swap_of_the_addend_differs(isa_same, tmp_path, capsys):
    rc, out = _pk(isa_same, tmp_path, capsys, "v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]", "v[4:5], v[8:9], v[6:7] op_sel_hi:[1,1,0]",
                  "--allow-commuted")
    assert rc == 1 and out == ["differs  _Z6kern_cPf (17 -> 17 lines, first at line 6 of the kernel)"]


def test_a_commuted_kernel_next_to_a_changed_one_still_fails(isa_same, tmp_path, capsys):
    old = [B, ("_Z6kern_cPf", PK)]
    new = [(B[0], B[1].replace("v1, v1, v2", "v1, v1, v3")),
           ("_Z6kern_cPf", PK.replace("v[4:5], v[6:7], v[8:9] op_sel_hi:[1,0,1]", "v[6:7], v[4:5], v[8:9] op_sel_hi:[0,1,1]"))]
    (tmp_path / "old.s").write_text(_file(old, "00"))
    (tmp_path / "new.s").write_text(_file(new, "00"))
    rc = isa_same.main(["isa_same.py", "--allow-commuted", str(tmp_path / "old.s"), str(tmp_path / "new.s")])
    out = capsys.readouterr().out.splitlines()
    assert rc == 1 and sorted(o.split()[0] for o in out) == ["commuted", "differs"]
