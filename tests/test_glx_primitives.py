"""Every function of the device branch of gl64_gfx950.cuh against unsigned __int128 arithmetic on the host.

GPU: tools/ubench/glx_check.hip applies each function once per element -- the edge grid of tools/ubench/gl_prims.hip crossed with
itself, the S-box inputs 2^48 / 2^24 / 2^14, random words, and for the products waves built with the model of the tail (one
borrow-only lane at lane 0 / 31 / 32 / 63, in each slot of glx_mul3, all lanes, lanes switched off, a partial last wave) -- and fails
if a class of a function's fix-up stays empty.  The test builds it, runs it once and wants one `ok` line per function.
CPU: a glx_* / Glx* name defined in the header's device branch that neither glx_check.hip nor wide_acc.hip mentions fails the
suite: a primitive added later cannot ship unchecked."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "plonky2_demo_amd", "csrc", "gl64_gfx950.cuh")
CHECKER = os.path.join(ROOT, "tools", "ubench", "glx_check.hip")
WIDE_ACC = os.path.join(ROOT, "tools", "ubench", "wide_acc.hip")

EXPECTED = (["glx_mul<false>", "glx_mul<true>", "glx_mul3<false>", "glx_mul3<true>", "glx_add_cc", "glx_sub_cc", "glx_sub_cc4", "glx_canon",
             "glx_add_eps_if", "glx_mk64", "glx_fix_canon", "glx_reduce96", "glx_acc_reduce", "glx_acc_reduce3", "glx_mad_k", "glx_mac_c"]
            + ["glx_shl_c<%d>" % e for e in range(1, 96)])


def device_branch(text):
    """the part of the header between `#if defined(__HIP_DEVICE_COMPILE__)` and its `#elif`"""
    start = text.index("#if defined(__HIP_DEVICE_COMPILE__)")
    return text[start:text.index("#elif defined(__HIPCC__)", start)]


def defined_names(branch):
    """functions (`glx_name(` after a return type at the start of a line), structs and typedefs"""
    names = set(re.findall(r"^(?:template <[^>]*>\s*)?__device__ __forceinline__ [\w:]+&? (glx_\w+)\(", branch, re.M))
    names |= set(re.findall(r"^struct (Glx\w+|glx_\w+)", branch, re.M))
    names |= set(re.findall(r"^typedef .*?\b(glx_\w+|Glx\w+)\b[^;]*;", branch, re.M))
    return names


def test_every_primitive_of_the_header_is_named_by_a_checker():
    branch = device_branch(open(HEADER).read())
    names = defined_names(branch)
    # the collection itself: what the header is known to define today is found, and nothing glx_* in the branch escapes the patterns
    assert {"glx_u32x2", "glx_mk64", "glx_add_eps_if", "glx_mul3", "glx_mul", "glx_mad_k", "glx_mac_c", "glx_reduce96", "glx_acc_reduce",
            "glx_acc_reduce3", "glx_canon", "glx_add_cc", "glx_sub_cc", "glx_sub_cc4", "glx_fix_canon", "glx_shl_c", "GlxWideAcc2"} <= names
    code = re.sub(r"//[^\n]*", "", branch)
    assert set(re.findall(r"\b(?:glx_|Glx)\w+", code)) == names
    # a call or a use, not a mention in a comment
    checked = re.sub(r"//[^\n]*", "", open(CHECKER).read() + open(WIDE_ACC).read())
    missing = sorted(n for n in names if not re.search(r"\b%s\b" % n, checked))
    assert not missing, "defined in gl64_gfx950.cuh, used by neither tools/ubench/glx_check.hip nor wide_acc.hip: %s" % ", ".join(missing)


def test_expected_lines_cover_what_the_checker_prints():
    # every name the test below waits for is one the checker's source can print
    src = open(CHECKER).read()
    for name in EXPECTED:
        base = name.split("<")[0]
        assert '"%s' % base in src, name


@pytest.mark.gpu
def test_header_primitives_against_int128(gpu):
    exe = os.path.join(ROOT, "tools", "ubench", "bin", "glx_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(CHECKER), os.path.getmtime(HEADER)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "plonky2_demo_amd", "csrc"), CHECKER, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and "MISMATCH" not in r.stdout, r.stdout
    lines = r.stdout.splitlines()
    for name in EXPECTED:
        assert sum(l.startswith(name + ": ok (") for l in lines) == 1, "no single ok line for %s\n%s" % (name, r.stdout)
    assert "failing functions: 0" in r.stdout
