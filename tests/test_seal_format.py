"""tests/seal_format.py against hashlib and against the fixtures Microsoft SEAL 4.1 wrote (tests/golden/seal_format/): the
compression function, parms_id, the expansion of every seeded object including rejected and re-rejected words, and the writer's
bytes.  The GPU tests are judged by the restatement that this file pins."""
import hashlib
import json
import os

import numpy as np
import pytest

import seal_format as SF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seal_format")


def _bytes(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _chain_ids(n, primes):
    """SEAL's parms_id of the key level and of every data level below it"""
    ids = {SF.parms_id(n, primes): len(primes)}
    for L in range(len(primes) - 1, 0, -1):
        ids[SF.parms_id(n, primes[:L])] = L
    return ids


@pytest.mark.parametrize("digest_size", [32, 64])
@pytest.mark.parametrize("key", [b"", bytes(range(64)), b"k" * 17])
@pytest.mark.parametrize("length", [0, 1, 64, 127, 128, 129, 256, 300])
def test_blake2b_matches_hashlib(length, key, digest_size):
    data = bytes((5 * i + 1) & 0xFF for i in range(length))
    assert SF.blake2b(data, digest_size, key) == hashlib.blake2b(data, digest_size=digest_size, key=key).digest()


def test_prng_root_is_keyed_blake2b_with_xof_length():
    """hashlib cannot set xof_length, but with xof_length = 0 the root is ordinary keyed BLAKE2b of the counter"""
    seed = bytes(range(64))
    assert SF.blake2b((7).to_bytes(8, "little"), 64, seed) == hashlib.blake2b((7).to_bytes(8, "little"), key=seed).digest()
    assert SF.prng_root(seed, 7) != SF.prng_root(seed, 7 + (1 << 32)) != SF.prng_root(seed, 7 + (1 << 33))


def test_prng_buffers_are_independent_of_batching():
    seed = bytes((3 * i + 2) & 0xFF for i in range(64))
    three = SF.prng_buffers(seed, 5, 3)
    assert len(three) == 3 * 4096
    assert three == b"".join(SF.prng_buffers(seed, 5 + c, 1) for c in range(3))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_parms_id_against_every_fixture_header(name):
    parms = SF.read_parms(_bytes(name + "_parms.bin"))
    info = _json(name + ".json")
    assert (parms["scheme"], parms["n"], parms["primes"], parms["plain_modulus"]) == (SF.SCHEME_CKKS, info["n"], info["primes"], 0)
    ids = _chain_ids(info["n"], info["primes"])
    k = len(info["primes"])
    seen = 0
    for f in sorted(os.listdir(GOLDEN)):
        if not f.startswith(name + "_") or not f.endswith(".bin") or "parms" in f:
            continue
        data = _bytes(f)
        if "_ct_" in f or "_pk_" in f:
            c = SF.read_ciphertext(data)
            assert ids[c["parms_id"]] == c["L"] == (k if "_pk_" in f else k - 1), f
        elif "_rk_" in f or "_gk_" in f:
            ks = SF.read_kswitch_keys(data)
            assert ids[ks["parms_id"]] == k, f
            assert all(ids[d["parms_id"]] == k for digits in ks["keys"] for d in digits), f
        else:
            p = SF.read_plaintext(data)
            assert ids[p["parms_id"]] * info["n"] == p["data"].size, f
        seen += 1
    assert seen >= 2


def _digits(ks):
    return [d for digits in ks["keys"] for d in digits]


@pytest.mark.parametrize("stem", ["a_ct", "a_pk", "c_ct"])
def test_expansion_of_seeded_ciphertexts(stem):
    info = _json(stem[0] + ".json")
    seeded, full = SF.read_ciphertext(_bytes(stem + "_seeded.bin")), SF.read_ciphertext(_bytes(stem + "_full.bin"))
    assert seeded["seed"] is not None and seeded["prng_type"] == SF.PRNG_BLAKE2XB and full["seed"] is None
    got, rejected = SF.expand_ciphertext(seeded, info["primes"])
    assert (got == full["data"]).all()
    if stem == "c_ct":
        assert rejected == [0, 0]  # CoeffModulus::Create primes: the ordinary case
    if stem == "a_ct":
        assert sum(rejected) >= 1  # the condition on the committed seeds of Set A


@pytest.mark.parametrize("stem", ["a_rk", "a_gk"])
def test_expansion_of_seeded_keys(stem):
    info = _json("a.json")
    seeded, full = SF.read_kswitch_keys(_bytes(stem + "_seeded.bin")), SF.read_kswitch_keys(_bytes(stem + "_full.bin"))
    assert [len(d) for d in seeded["keys"]] == [len(d) for d in full["keys"]]
    k = len(info["primes"])
    assert len(_digits(seeded)) == (k - 1) * (1 if stem == "a_rk" else 2)
    if stem == "a_gk":
        # SEAL/galoiskeys.h: slot (elt - 1) / 2 for the Galois elements of steps 1 and 3, 5^1 and 5^3 mod 2N
        assert [i for i, d in enumerate(seeded["keys"]) if d] == sorted([(5 - 1) // 2, (125 - 1) // 2])
    for s, f in zip(_digits(seeded), _digits(full)):
        got, _ = SF.expand_ciphertext(s, info["primes"])
        assert (got == f["data"]).all()


def test_set_b_expansion_against_digests_and_rerejection():
    info = _json("b.json")
    primes = info["primes"]
    ct = SF.read_ciphertext(_bytes("b_ct_seeded.bin"))
    got, rejected = SF.expand_ciphertext(ct, primes)
    assert hashlib.sha256(got.astype("<u8").tobytes()).hexdigest() == info["ct_sha256"]
    # the condition on the committed seeds of Set B: a replacement word that is itself rejected, i.e. more rejections than
    # rejected candidates among the first L N words
    first = np.frombuffer(SF.prng_buffers(ct["seed"], 0, 4), dtype="<u8")[:2 * 1024].reshape(2, 1024)
    candidates = [int((first[j] >= np.uint64(SF.max_multiple(primes[j]))).sum()) for j in range(2)]
    assert sum(rejected) > sum(candidates) >= 1, (rejected, candidates)
    rk = SF.read_kswitch_keys(_bytes("b_rk_seeded.bin"))
    words = b"".join(SF.expand_ciphertext(d, primes)[0].astype("<u8").tobytes() for d in _digits(rk))
    assert hashlib.sha256(words).hexdigest() == info["rk_sha256"]


def test_writer_reproduces_every_full_fixture():
    for name in ("a", "b", "c"):
        info = _json(name + ".json")
        assert SF.write_parms(info["n"], info["primes"]) == _bytes(name + "_parms.bin")
    for f in ("a_ct_full.bin", "a_pk_full.bin", "c_ct_full.bin", "a_ct_seeded.bin", "c_ct_seeded.bin"):
        c = SF.read_ciphertext(_bytes(f))
        assert SF.write_ciphertext(c["parms_id"], c["ntt"], c["size"], c["n"], c["L"], c["scale"], c["data"], c["seed"],
                                   c["correction_factor"]) == _bytes(f), f
    for f in ("a_pt.bin", "a_sk.bin"):
        p = SF.read_plaintext(_bytes(f))
        assert SF.write_plaintext(p["parms_id"], p["scale"], p["data"]) == _bytes(f), f
    for f in ("a_rk_full.bin", "a_gk_full.bin"):
        ks = SF.read_kswitch_keys(_bytes(f))
        keys = [[SF.write_ciphertext(d["parms_id"], d["ntt"], d["size"], d["n"], d["L"], d["scale"], d["data"]) for d in digits]
                for digits in ks["keys"]]
        assert SF.write_kswitch_keys(ks["parms_id"], keys) == _bytes(f), f


def test_reader_rejects_what_seal_rejects():
    data = bytearray(_bytes("a_ct_seeded.bin"))
    for at, value, message in ((0, 0x5F, "invalid"), (3, 5, "incompatible version"), (5, 1, "invalid"), (5, 2, "invalid")):
        bad = bytearray(data)
        bad[at] = value
        with pytest.raises(ValueError, match=message):
            SF.read_ciphertext(bytes(bad))
    with pytest.raises(ValueError, match="I/O error"):
        SF.read_ciphertext(bytes(data[:-1]))


def test_fixture_sizes():
    sizes = [os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)]
    assert max(sizes) <= 128 * 1024 and sum(sizes) <= 400 * 1024
    # SEAL's own count for a seeded ciphertext at N = 1024, L = 2: header, members, one polynomial, generator info
    assert len(_bytes("b_ct_seeded.bin")) == 16 + 73 + (16 + 8 + 16384) + (16 + 1 + 64) == 16578
