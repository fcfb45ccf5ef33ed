"""The seal:: C++ surface (moai-fhe-transformerinference-public_amd/seal_shim) over the C ABI.

CPU: the shim and MOAI's own headers compile together (the reference checkout is only present in the
build container, so that part is skipped elsewhere).  GPU: the prebuilt C++ test binaries run the
reference-style encode -> encrypt -> evaluate -> decrypt -> decode checks and MOAI's unchanged
matrix-mul / GELU headers on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
CPP = os.path.join(ROOT, "tests", "cpp")
REF = "/root/reference/include/source"


def _gxx(args, **kw):
    return subprocess.run(["g++", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "seal_shim")] + args, capture_output=True, text=True, **kw)


def test_shim_compiles_standalone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "seal/seal.h"\nint main() { seal::EncryptionParameters p(seal::scheme_type::ckks); return 0; }\n')
    r = _gxx(["-fsyntax-only", str(src)])
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present on this machine")
def test_moai_headers_compile_unchanged_against_shim(tmp_path):
    """include/include.hpp's header list minus the NTL-dependent bootstrapping."""
    src = tmp_path / "moai.cpp"
    src.write_text(
        '#include "seal/seal.h"\n#include <omp.h>\n#include <sys/time.h>\n#include <chrono>\n#include <cmath>\n'
        "#include <fstream>\n#include <iomanip>\n#include <iostream>\n#include <vector>\n"
        '#include "Batch_encode_encrypt.hpp"\n#include "Ct_pt_matrix_mul.hpp"\n#include "Ct_ct_matrix_mul.hpp"\n'
        '#include "layernorm.hpp"\n#include "gelu.hpp"\n#include "gelu_others.hpp"\nint main() { return 0; }\n'
    )
    r = _gxx(["-fsyntax-only", "-I" + REF + "/matrix_mul", "-I" + REF + "/non_linear_func", str(src)])
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_test_binaries_are_built():
    # built by __graft_entry__.build() (make -C tests/cpp); they travel to the GPU box with the snapshot
    assert os.path.exists(os.path.join(CPP, "test_seal_shim"))
    if os.path.isdir(REF):  # it includes MOAI's own headers: built only where they are (tests/cpp/Makefile)
        assert os.path.exists(os.path.join(CPP, "test_moai_headers"))
    assert os.path.exists(os.path.join(CPP, "test_bootstrap_lt"))
    assert os.path.exists(os.path.join(CPP, "test_bootstrap_eval"))
    assert os.path.exists(os.path.join(CPP, "test_bootstrap_setup"))
    assert os.path.exists(os.path.join(CPP, "test_bootstrap_real"))


def test_bootstrap_polynomial_heap_host_checks():
    """babycount, the quotient / remainder heap of the modular-reduction polynomial and the rotation-key list:
    host arithmetic only (tests/cpp/test_bootstrap_eval.cpp, part 1); the device parts run under -m gpu."""
    r = subprocess.run([os.path.join(CPP, "test_bootstrap_eval"), "--host-only"], cwd=CPP, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASS" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


def test_bootstrap_setup_constants_host_checks():
    """The bootstrapping constants are re-derived without NTL (seal_shim/bootstrapping/moai_remez.h, moai_fft_diagonals.h).
    Host-only: equioscillation of the minimax cosine / inverse sine, F P = U and G F = identity / 2K for the diagonals
    (tests/cpp/test_bootstrap_setup.cpp), and the cosine's coefficients against an independent 400-bit computation of
    the same polynomial (tests/golden/remez_cos_K25_deg59_loge10_r2.json, written by tools/remez_mpmath.py)."""
    import json

    exe = os.path.join(CPP, "test_bootstrap_setup")
    r = subprocess.run([exe], cwd=CPP, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASS" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "remez_cos_K25_deg59_loge10_r2.json")))
    r = subprocess.run([exe, "--print-cos", str(gold["boundary_K"]), str(gold["log_width"]), str(gold["deg"]), str(gold["scale_factor"])],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    vals = [float(x) for x in r.stdout.split()]
    want = [float(x) for x in gold["chebcoeff"]]
    assert abs(vals[0] - float(gold["minimax_error"])) < 1e-22
    assert len(vals) == len(want) + 1
    # as doubles: equal to the last place or one off it
    for got, w in zip(vals[1:], want):
        assert abs(got - w) <= 2.3e-16 * abs(w), (got, w)


@pytest.mark.gpu
@pytest.mark.parametrize("binary", ["test_seal_shim", "test_moai_headers", "test_moai_attention", "test_bootstrap_lt", "test_bootstrap_eval",
                                    "test_bootstrap_real", "test_moai_drivers", "test_moai_fixtures"])
def test_cpp_binary_passes_on_gpu(binary):
    """test_moai_headers / test_moai_attention include MOAI's own headers from the reference checkout at build time (the
    binaries travel prebuilt); test_moai_attention is MOAI's single_att_block + softmax_boot unchanged, checked by decryption;
    test_moai_drivers = the three weight-free drivers the reference's test.cpp:18-30 calls, through its include.hpp, printed slots
    asserted against their closed forms; test_moai_fixtures = MOAI's Q K^T / softmax_boot / . V / layernorm / layernorm2 /
    gelu_v2 at N = 2^16 on the 36-prime chain against the reference's own activation fixtures (tests/golden/moai_data)"""
    if binary.startswith("test_moai_") and not os.path.exists(os.path.join(CPP, binary)) and not os.path.isdir(REF):
        pytest.skip("built from MOAI's own headers, which only the build container holds")
    r = subprocess.run([os.path.join(CPP, binary)], cwd=CPP, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL PASS" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_bootstrap_returns_the_message_at_moai_parameters():
    """decrypt(bootstrap_3(ct)) = message at N = 2^16 on MOAI's 36-prime chain with the constants of
    include/test/test_full_scheme.hpp:345-448 (K = 25, degree 59, level-3 transforms): chain index 0 -> 20, error below 1e-4,
    a pack of 2 bit-identical to two single runs (tests/cpp/test_bootstrap_real.cpp --full)"""
    r = subprocess.run([os.path.join(CPP, "test_bootstrap_real"), "--full", "8", "2"], cwd=CPP, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ALL PASS" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


def test_client_randomness_is_a_chacha20_stream(tmp_path):
    """seal::KeyGenerator / Encryptor draw from ChaCha20 keyed by the OS (moai_client.h).  Known answer: the first block
    of the all-zero key and nonce (draft-agl-tls-chacha20poly1305-04 section 7, test vector 1), and two generators
    seeded from the OS do not repeat each other."""
    src = tmp_path / "rng.cpp"
    src.write_text(r'''
#include "seal/seal.h"
#include <cstdio>
int main() {
    unsigned char seed[40] = {0};
    seal::util::ChaCha20Rng g(seed);
    for (int i = 0; i < 8; i++) { unsigned long long v = g(); for (int b = 0; b < 8; b++) std::printf("%02x", (unsigned)((v >> (8 * b)) & 0xff)); }
    std::printf("\n");
    seal::util::ChaCha20Rng a, b;
    std::printf("%d\n", a() == b() ? 1 : 0);
    return 0;
}
''')
    exe = tmp_path / "rng"
    r = _gxx([str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split()
    assert lines[0] == ("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
                        "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586")
    assert lines[1] == "0"


def test_key_plan_orders_slots_and_refuses_bad_elements(tmp_path):
    """seal::util::galois_key_plan (moai_client.h): what KeyGenerator::create_*_keys generates and in which order, host
    arithmetic without a context.  n = 8, k = 4: elements 1, 3 .. 15 are slots 0 .. 7, and levels_of saturates at chain index 2."""
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#include "seal/seal.h"
#include <cstdio>
using namespace seal::util;
static int bad = 0;
static void check(bool ok, const char *what) { if (!ok) { std::printf("FAIL %s\n", what); bad++; } }
template <class F> static std::string refusal(F f)
{
    try { f(); } catch (const std::invalid_argument &e) { return e.what(); } catch (...) { return "another exception"; }
    return "no exception";
}
int main() {
    const std::size_t n = 8, k = 4;
    check(levels_of(0, k) == 1 && levels_of(1, k) == 2, "levels_of below the top: chain index + 1");
    check(levels_of(k - 2, k) == k - 1 && levels_of(k, k) == k - 1 && levels_of(k - 2, k) == levels_of(k, k), "levels_of saturates at k-1");
    // the given order, not the order of the slots; 11 again is dropped, with the levels of its first mention
    const std::vector<std::uint32_t> elts = { 11, 3, 15, 11, 1 };
    const std::vector<std::size_t> each = { 0, 1, 2, 1, 5 };
    check(galois_key_plan(elts, &each, n, k) == KeyPlan{ { 5, 1 }, { 1, 2 }, { 7, 3 }, { 0, 3 } }, "per-element chain indices");
    const std::vector<std::size_t> one = { 1 };
    check(galois_key_plan(elts, &one, n, k) == KeyPlan{ { 5, 2 }, { 1, 2 }, { 7, 2 }, { 0, 2 } }, "one chain index for all elements");
    check(galois_key_plan(elts, nullptr, n, k) == KeyPlan{ { 5, 3 }, { 1, 3 }, { 7, 3 }, { 0, 3 } }, "whole keys: k-1 levels");
    check(galois_key_plan({}, nullptr, n, k).empty() && galois_key_plan({}, &one, n, k).empty(), "no elements, no keys");
    const std::vector<std::size_t> four = { 0, 1, 2, 1 }, none = {};
    const std::string count = "chain_indices must hold one entry, or one per Galois element", elt = "Galois element is not valid";
    check(refusal([&] { galois_key_plan(elts, &four, n, k); }) == count, "four chain indices for five elements");
    check(refusal([&] { galois_key_plan(elts, &none, n, k); }) == count, "no chain index for five elements");
    check(refusal([&] { galois_key_plan({ 3, 4 }, nullptr, n, k); }) == elt, "an even element");
    check(refusal([&] { galois_key_plan({ 3, 0 }, &one, n, k); }) == elt, "element 0");
    check(refusal([&] { galois_key_plan({ 3, 2 * n }, nullptr, n, k); }) == elt, "element 2n");
    check(refusal([&] { galois_key_plan({ 3, 2 * n + 1 }, nullptr, n, k); }) == elt, "element 2n + 1");
    check(galois_key_plan({ 2 * n - 1 }, nullptr, n, k) == KeyPlan{ { n - 1, 3 } }, "element 2n - 1 is the last slot");
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
''')
    exe = tmp_path / "plan"
    r = _gxx([str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "bad 0" in out.stdout, (out.stdout[-3000:], out.stderr[-2000:])
