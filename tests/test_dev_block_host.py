"""CPU: the owner of libaoenv's device memory (rlao_amd/csrc/dev_block.hpp) on host memory with a counting allocator, in the
stand-alone program tests/native/dev_block_driver.cpp -- once plain, once under AddressSanitizer and UBSan -- and the guard for the
next feature: rlao_amd/csrc/env.hip allocates and frees device memory through the owner alone.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_HIP = os.path.join(REPO, "rlao_amd", "csrc", "env.hip")

# what the driver answers, line by line
EXPECTED = """\
layout_offsets null 0 256 512 768
layout_total 1280
parts_rc 0 calls 1 live 1
parts_from_base null 0 256 512 768
parts_outside 1 1
base_misaligned 0
zeros_only rc 0 allocations 0 live_block 0 part0_null 1
zeroed_nonzero_bytes 0
unzeroed_touched_bytes 0
upload ok 0 too_long 1 absent 1 empty 0 arrived 1 next_part_untouched 0
failed_alloc rc 1 empty 1 part0_null 1 live_delta 0
failed_replacement rc 1 same_block 1 data_intact 1 frees 0 live_delta 1
replacement rc 0 old_freed 1 frees 1 live_delta 1
move_construct frees 0 source_empty 1 dest_holds 1 frees_after_scope 1
move_assign frees 1 target_old_freed 1 target_holds_source 1 source_empty 1 frees_after_scope 2
self_move_assign frees 0 still_holds 1 frees_after_scope 1
reset_twice frees 1 empty 1 frees_after_scope 1
record_move frees 1 old_freed 1 holds_new 1 K 7 set 1 local_block_empty 1 frees_after_scope 1 live_delta 1
record_clear frees 2 live_delta 0 set 0 K 0 pointers_null 1 block_empty 1
exit live 0 bad_frees 0 allocations 13 frees 13
""".splitlines()


def build_driver(out_dir, sanitize):
    """Compiles tests/native/dev_block_driver.cpp for the host (as tests/_policy_ref.py builds its driver); None without hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "dev_block_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "dev_block_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_driver_answers(tmp_path, sanitize):
    """Layout ({0, 1, 255, 256, 257} -> null, 0, 256, 512, 768; 1280 bytes; zeros alone allocate nothing), zeroing, a failed
    allocation (empty / the block to be replaced intact, live count unchanged), every way a block is freed exactly once, the record
    swap of the feature code.  Sanitized: a clean exit and no report as well."""
    exe = build_driver(tmp_path, sanitize)
    if exe is None:
        pytest.skip("no hipcc")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.splitlines() == EXPECTED
    if sanitize:
        assert "ERROR: AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_header_compiles_as_plain_cpp(tmp_path):
    """dev_block.hpp holds no HIP: a translation unit that includes it alone compiles as C++ with -Wall -Wextra -Werror."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (os.path.exists(cxx) or shutil.which(cxx)):
        pytest.skip("no host C++ compiler")
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "dev_block.hpp"\nint main() { return ao::dev_layout({1, 0, 257}).total == 768 ? 0 : 1; }\n')
    exe = tmp_path / "only_header"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{REPO}/rlao_amd/csrc", str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    assert subprocess.run([str(exe)]).returncode == 0
    text = open(os.path.join(REPO, "rlao_amd", "csrc", "dev_block.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", text)


# ---- env.hip ----------------------------------------------------------------------------------------------------------------------
def _braced(src, start):
    """the text of the brace block that opens at or after `start`, and the index behind it"""
    i = src.index("{", start)
    depth = 0
    for j in range(i, len(src)):
        depth += (src[j] == "{") - (src[j] == "}")
        if depth == 0:
            return src[i:j + 1], j + 1
    raise AssertionError("unbalanced braces")


def test_env_hip_allocates_through_the_owner_alone():
    """hipMalloc( and hipFree( occur in env.hip inside the owner's HIP policy (struct HipMem) and nowhere else, once each."""
    src = open(ENV_HIP).read()
    start = src.index("struct HipMem")
    policy, end = _braced(src, start)
    assert policy.count("hipMalloc(") == 1 and policy.count("hipFree(") == 1, policy
    rest = src[:start] + src[end:]
    for call in ("hipMalloc(", "hipFree(", "hipMallocAsync(", "hipFreeAsync(", "hipMallocManaged(", "hipHostMalloc("):
        assert call not in rest, f"{call} outside struct HipMem: device memory goes through DevBlock (dev_block.hpp)"
    assert "DevBlock<HipMem>" in src


def test_aoenv_destroy_names_no_feature_record():
    """aoenv_destroy is the device guard, the profiling events and `delete env`: every member frees itself, so a new feature has no
    line to forget there."""
    src = open(ENV_HIP).read()
    body, _ = _braced(src, src.index("int aoenv_destroy(AoEnv* env)"))
    named = set(re.findall(r"env->(\w+)", body))                   # every member of the env the function touches
    assert named == {"device", "prof_ev"}, named
    assert "DeviceGuard" in body and "delete env;" in body and "hipEventDestroy" in body
    assert body.index("DeviceGuard") < body.index("delete env;")   # the blocks are freed on the env's device
