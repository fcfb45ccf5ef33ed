"""CPU-only checks of the SEAL-seeded generating side: the header declares and cites the two entry points and documents the
seed's nonce purpose, hip.py binds them, and the seal:: shim's host half -- the opt-in switch on util::DeviceRng and the
64-byte seeds it derives (purpose 6 of the stream contract) -- against tests/client_sampling.py's ChaCha20 stream."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import client_sampling as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")
NAMES = ("moai_encrypt_symmetric_seal_seeded", "moai_kswitch_keygen_seal_seeded")


def _declaration_with_comment(hdr, name):
    at = hdr.index("int %s(" % name)
    start = hdr.rfind("/*", 0, at)
    # the comment must belong to this declaration: no other declaration in between
    assert ";" not in hdr[hdr.index("*/", start):at], name
    return hdr[start:at]


def test_header_declares_and_cites_the_entry_points(moai):
    hdr = open(os.path.join(ROOT, "include", "moai_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
    enc, key = (_declaration_with_comment(hdr, name) for name in NAMES)
    assert "SEAL/util/rlwe.cpp:311-385" in enc and "SEAL/ciphertext.cpp:118-151" in enc
    assert "SEAL/keygenerator.cpp:303-336" in key
    # the stream contract names the purpose the seeds are drawn under
    assert re.search(r"purpose 6\s+SEAL seed", hdr)
    L = C.CDLL(moai.lib_path())
    assert all(hasattr(L, name) for name in NAMES)


def test_binding_types_the_entry_points(moai):
    vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
    S = moai.hip.SYMBOLS
    assert S[NAMES[0]] == (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, vp, sz, sz, u32p, vp, vp])
    assert S[NAMES[1]] == (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, vp, vp, vp])
    lib = moai.hip.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes == S[name][1]
    assert callable(moai.Context.encrypt_symmetric_seal_seeded) and callable(moai.Context.kswitch_keygen_seal_seeded)
    # validated before the device is touched
    assert lib.moai_encrypt_symmetric_seal_seeded(None, bytes(32), bytes(64), 0, None, None, None, 1, 1, None, None, None) == moai.hip.MOAI_EINVAL
    assert b"null context" in lib.moai_last_error()
    assert lib.moai_kswitch_keygen_seal_seeded(None, bytes(32), bytes(64), 0, None, None, None, None, None) == moai.hip.MOAI_EINVAL


PROGRAM = r"""
#include <cstdio>
#include "seal/seal.h"
using namespace seal;
int main()
{
    unsigned char key[32];
    for (int i = 0; i < 32; i++) key[i] = (unsigned char)(5 * i + 2);
    util::DeviceRng rng(key, 40);
    std::printf("default %d\n", rng.get_seed_kind() == seed_kind::chacha20);
    rng.set_seed_kind(seed_kind::seal_blake2xb);
    std::printf("switched %d\n", rng.get_seed_kind() == util::seed_kind::seal_blake2xb);
    // the switch reserves nothing: sequences are handed out as before
    const unsigned long long first = rng.take(3), second = rng.take(1);
    std::printf("take %llu %llu\n", first, second);
    const std::vector<std::uint8_t> seeds = util::seal_seeds(rng.key(), (std::uint64_t(1) << 40) + 7, 2);
    std::printf("seeds ");
    for (std::uint8_t b : seeds) std::printf("%02x", b);
    std::printf("\n");
    std::uint8_t pub[32];
    util::public_seed(rng.key(), 9, pub);
    std::printf("public ");
    for (std::uint8_t b : pub) std::printf("%02x", b);
    std::printf("\n");
    return 0;
}
"""


def _stream_head(key, purpose, seq, words):
    return CS.words(key, CS.nonce(purpose, seq), 0, 1)[:words].astype("<u8").tobytes().hex()


def test_shim_switch_and_seed_derivation(moai, tmp_path):
    src = tmp_path / "seal_seeds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "seal_seeds"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(PKG, "seal_shim"), str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    out = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    assert out["default"] == "1" and out["switched"] == "1" and out["take"] == "40 43"
    key = bytes((5 * i + 2) & 0xFF for i in range(32))
    seq = (1 << 40) + 7
    # W[0..7] of (noise key, 6 << 56 | seq + b), little endian, one block each
    assert out["seeds"] == _stream_head(key, 6, seq, 8) + _stream_head(key, 6, seq + 1, 8)
    # purpose 5 is what it was: the first 32 bytes of its stream
    assert out["public"] == _stream_head(key, 5, 9, 4)
    assert np.frombuffer(bytes.fromhex(out["seeds"]), dtype=np.uint8).size == 128
