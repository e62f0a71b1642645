"""The planner's workspace arena (csrc/xv_arena.h: first fit, carved from the front, free list sorted by offset, adjacent
blocks merged) on the host: tests/host/arena_check.cpp replays three hand-written sequences and drives seeded random
alloc / release sequences, checking after every call that live blocks neither overlap nor reach past top(), that the free
list is sorted, merged and disjoint from them, and that releasing everything leaves one block [0, top()).  Built with
AddressSanitizer and UBSan and run directly: a plain host program, nothing is loaded into Python."""
import os
import subprocess


def test_arena_invariants_under_asan_and_ubsan(tmp_path, repo_root):
    exe = str(tmp_path / "arena_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(repo_root, "tf-kaldi-speaker_amd", "csrc"),
                    os.path.join(repo_root, "tests", "host", "arena_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "arena ok"
