"""Pins the comparator tests/client_sampling.py (the stream contract of include/moai_hip.h, "client randomness and
encryption") three ways: the all-zero-key ChaCha20 vector test_seal_shim.py already uses, the host
seal::util::ChaCha20Rng(seed) on non-zero seeds, and hand-checked cases of every sampler mapping.  CPU only."""
import os
import subprocess

import numpy as np

import client_sampling as CS
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")

# draft-agl-tls-chacha20poly1305-04 section 7, test vector 1: all-zero key and nonce, block 0
ZERO_BLOCK = ("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
              "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586")


def _hex_le(ws):
    return "".join(int(w).to_bytes(8, "little").hex() for w in ws)


def test_zero_key_vector():
    assert _hex_le(CS.words(bytes(32), 0, 0, 1)) == ZERO_BLOCK
    # the block function takes any counter: block 1 of the same stream is the next 8 words
    assert (CS.words(bytes(32), 0, 0, 2)[8:] == CS.words(bytes(32), 0, 1, 1)).all()


def test_matches_host_chacha20rng(tmp_path):
    """seal::util::ChaCha20Rng(key || nonce) gives word for word the stream of (key, nonce), across block boundaries and
    with a nonce that uses both of its 32-bit halves"""
    src = tmp_path / "rng.cpp"
    src.write_text(r'''
#include "seal/seal.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    unsigned char seed[40];
    for (int i = 0; i < 40; i++) seed[i] = (unsigned char)(std::strtoul(argv[1], nullptr, 10) * 37 + i * 11 + 1);
    seal::util::ChaCha20Rng g(seed);
    for (int i = 0; i < 40; i++) std::printf("%llu\n", (unsigned long long)g());
    return 0;
}
''')
    exe = tmp_path / "rng"
    r = subprocess.run(["g++", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(PKG, "seal_shim"), str(src), "-o", str(exe), "-L" + PKG, "-lmoai_hip",
                        "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for s in (1, 5):
        seed = bytes((s * 37 + i * 11 + 1) & 0xFF for i in range(40))
        out = subprocess.run([str(exe), str(s)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        host = np.array([int(x) for x in out.stdout.split()], dtype=np.uint64)
        nonce = int.from_bytes(seed[32:], "little")
        assert nonce >> 32 and nonce & 0xFFFFFFFF
        assert (CS.words(seed[:32], nonce, 0, 5) == host).all()


def test_uniform_mapping_by_hand():
    q = 0x3FFFFFFFFF000001  # a 62-bit odd modulus
    lo = np.array([0, 5, 2**64 - 1, 123456789, 0], dtype=np.uint64)
    hi = np.array([0, 0, 0, 1, 2**64 - 1], dtype=np.uint64)
    want = [0, 5, (2**64 - 1) % q, (2**64 + 123456789) % q, ((2**64 - 1) << 64) % q]
    assert [int(x) for x in CS.map_uniform(lo, hi, q)] == want
    # the stream layout: row r, coefficient i takes words 2 (r N + i) (low) and 2 (r N + i) + 1 (high)
    key, n, primes = bytes(range(32)), 8, [97, 193, 257]
    u = CS.uniform(key, 9, primes, n)
    w = CS.words(key, 9, 0, len(primes) * n // 4)
    for r, q in enumerate(primes):
        for i in range(n):
            f = r * n + i
            assert int(u[r, i]) == ((int(w[2 * f + 1]) << 64) + int(w[2 * f])) % q
    # computing selected rows gives the same rows
    part = CS.uniform(key, 9, primes, n, rows=[2])
    assert (part[2] == u[2]).all() and not part[0].any()


def test_ternary_mapping_by_hand():
    w = np.array([0, 2**64 // 3, 2**64 // 3 + 1, 2**63, (2**64 * 2) // 3 + 1, 2**64 - 1], dtype=np.uint64)
    assert list(CS.map_ternary(w)) == [-1, -1, 0, 0, 1, 1]


def test_cbd_mapping_by_hand():
    w = np.array([0, 0x1FFFFF, 0x1FFFFF << 24, 0xE00000, 0xE0 << 40, 0xFFFFFFFFFFFFFFFF, 0x010101, 0x020000 << 24,
                  0xFFFF000000000000], dtype=np.uint64)
    # bytes 6 and 7 are never read; bits 5-7 of bytes 2 and 5 are masked
    assert list(CS.map_cbd(w)) == [0, 21, -21, 0, 0, 0, 3, -1, 0]
    # the distribution of all 2^16 values of (x0, x3) with the others zero: popcount difference
    v = np.arange(1 << 16, dtype=np.uint64)
    x0, x3 = v & np.uint64(0xFF), v >> np.uint64(8)
    got = CS.map_cbd(x0 | (x3 << np.uint64(24)))
    want = np.array([bin(int(a)).count("1") - bin(int(b)).count("1") for a, b in zip(x0, x3)])
    assert (got == want).all()


def test_rns_of_small_samples():
    primes = [97, 2**61 - 1]
    got = CS.to_rns([-21, -1, 0, 1, 21], primes)
    assert [int(x) for x in got[0]] == [76, 96, 0, 1, 21]
    assert [int(x) for x in got[1]] == [2**61 - 22, 2**61 - 2, 0, 1, 21]


def test_sampler_distributions_are_sane():
    key = bytes(range(100, 132))
    n = 1 << 14
    e = CS.cbd(key, CS.nonce(CS.NOISE0, 0), n)
    assert e.min() >= -21 and e.max() <= 21 and abs(e.std() - np.sqrt(10.5)) < 0.1 and abs(e.mean()) < 0.1
    t = CS.ternary(key, CS.nonce(CS.TERNARY, 0), n)
    counts = np.bincount(t + 1, minlength=3)
    assert set(np.unique(t)) <= {-1, 0, 1} and (abs(counts - n / 3) < 5 * np.sqrt(n)).all()


def test_compositions_decrypt_to_small_noise():
    """symmetric: c0 + c1 s = e exactly; asymmetric after the division: |c0 + c1 s| <= ||s||_1 / 2 + 2; key digit J:
    c0 + c1 s = e + (p mod q_J) s' in row J"""
    logn, bits = 4, [30, 31, 32, 33]
    n = 1 << logn
    primes = O.coeff_modulus_create(n, bits)
    octx = O.Context(logn, primes)
    k = len(primes)
    rng = np.random.default_rng(3)
    s = rng.integers(-1, 2, size=n)
    s_ntt = octx.ntt(CS.to_rns(s, primes), k)
    key = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))

    def dec(ct, L):
        m = np.empty((L, n), dtype=np.uint64)
        for r in range(L):
            m[r] = ((ct[0, r].astype(object) + ct[1, r].astype(object) * s_ntt[r].astype(object)) % primes[r]).astype(np.uint64)
        coeff = octx.ntt(m, L, inverse=True)
        Q = 1
        for q in primes[:L]:
            Q *= q
        x = np.zeros(n, dtype=object)
        for r, q in enumerate(primes[:L]):
            Qi = Q // q
            x = x + coeff[r].astype(object) * (Qi * pow(Qi % q, -1, q))
        x = x % Q
        return np.array([int(v) - Q if v > Q // 2 else int(v) for v in x], dtype=object)

    ct = CS.encrypt_symmetric(octx, key, 7, s_ntt, 3)[0]
    assert list(dec(ct, 3)) == list(CS.cbd(key, CS.nonce(CS.NOISE0, 7), n))
    pk = CS.encrypt_symmetric(octx, key, 100, s_ntt, k)[0]
    bound = np.abs(s).sum() / 2 + 2
    for L in (k, k - 1, 2):
        ct = CS.encrypt_asymmetric(octx, key, 8, pk, L)[0]
        assert max(abs(v) for v in dec(ct, L)) <= (bound if L < k else 1e9)
    s2 = octx.ntt(CS.to_rns(s * 0 + 1, primes), k)
    for J in range(k - 1):
        d = CS.kswitch_digit(octx, key, 50, s_ntt, s2, J)
        m = np.empty((k, n), dtype=np.uint64)
        for r in range(k):
            m[r] = ((d[0, r].astype(object) + d[1, r].astype(object) * s_ntt[r].astype(object)) % primes[r]).astype(np.uint64)
        e = CS.to_rns(CS.cbd(key, CS.nonce(CS.NOISE0, 50 + J), n), primes)
        e = octx.ntt(e, k)
        f = primes[k - 1] % primes[J]
        for r in range(k):
            want = e[r].astype(object) + (s2[r].astype(object) * f if r == J else 0)
            assert (m[r] == (want % primes[r]).astype(np.uint64)).all()
