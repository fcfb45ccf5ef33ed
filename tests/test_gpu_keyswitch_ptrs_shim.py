"""Key switches on a list of ciphertexts on the seal:: surface (seal/moai_combiner.h, util::rot_resolve): one compiled program,
N = 2^12, chain {60, 40, 40, 60}, Galois keys for the steps 1, 2, 3, 4.  The first process makes the secret key, the keys and
eight inputs and saves them; it and three more run the same work under the four settings of the shim's knobs -- combining off,
the default, MOAI_SHIM_COMBINE_ANY_KEY=1, and the latter under MOAI_STREAM_AUDIT=1 -- and write what they computed: the files
must hold identical words.  The shim's knobs are read once per process, hence the processes.  A second, host-only program
checks the cap on a combiner group with a stub in the leader's place."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")

PROGRAM = r"""
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "seal/seal.h"
#include "seal/moai_fused.h"
using namespace seal;
static int bad = 0;
static void check(bool ok, const char *what) { if (!ok) { std::printf("FAIL %s\n", what); bad++; } }
static std::vector<seal_byte> read_file(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<seal_byte> b(s.size());
    std::memcpy(b.data(), s.data(), s.size());
    return b;
}
template <class T> static void to_file(const T &x, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    x.save(f);
}
template <class T> static void from_file(const SEALContext &c, T &x, const std::string &path)
{
    auto b = read_file(path);
    check(static_cast<std::size_t>(x.load(c, b.data(), b.size())) == b.size(), "load consumes the file");
}
template <class E, class F> static bool throws(F f)
{
    try { f(); } catch (const E &) { return true; } catch (...) { return false; }
    return false;
}
// units the census holds for (name, L)
static unsigned long long traced(const char *name, std::size_t L)
{
    std::vector<char> buf(moai_op_trace_dump(nullptr, 0) + 16);
    moai_op_trace_dump(buf.data(), buf.size());
    const std::string text(buf.data()), want = std::string(name) + " " + std::to_string(L) + " ";
    std::size_t at = 0;
    while (at < text.size())
    {
        std::size_t end = text.find('\n', at);
        end = end == std::string::npos ? text.size() : end;
        if (text.compare(at, want.size(), want) == 0) return std::stoull(text.substr(at + want.size(), end - at - want.size()));
        at = end + 1;
    }
    return 0;
}
using Words = std::vector<std::uint64_t>;
static void append(Words &w, const Words &x) { w.insert(w.end(), x.begin(), x.end()); }

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : ".", tag = argc > 3 ? argv[3] : "x";
    const char *env_any = std::getenv("MOAI_SHIM_COMBINE_ANY_KEY"), *env_us = std::getenv("MOAI_SHIM_COMBINE_US");
    const bool any_key = env_any && env_any[0] == '1', combining = !(env_us && std::atol(env_us) == 0);
    check(util::combine_any_key() == any_key, "the knob is read from the environment");
    const std::size_t n = 1 << 12;
    const int T = 8;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(CoeffModulus::Create(n, { 60, 40, 40, 60 }));
    SEALContext context(parms, true, sec_level_type::none);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context, encoder);
    const double scale = std::pow(2.0, 40);
    std::vector<std::uint32_t> elts;
    for (int step = 1; step <= 4; step++) elts.push_back(moai_galois_elt_from_step(context.device(), step));
    if (mode == "setup")
    {
        {
            KeyGenerator fresh(context);
            to_file(fresh.secret_key(), dir + "/sk.bin");
        }
        SecretKey sk;
        from_file(context, sk, dir + "/sk.bin");
        KeyGenerator gen(context, sk);
        to_file(gen.create_relin_keys(), dir + "/rk.bin");
        to_file(gen.create_galois_keys(elts), dir + "/gk.bin");
        Encryptor sym(context, sk);
        for (int t = 0; t < T; t++)
        {
            std::vector<double> v(encoder.slot_count());
            for (std::size_t s = 0; s < v.size(); s++) v[s] = 0.01 * t + 1e-4 * (double)(s % 97);
            Plaintext p;
            encoder.encode(v, scale, p);
            Ciphertext c;
            sym.encrypt_symmetric(p, c);
            to_file(c, dir + "/in" + std::to_string(t) + ".bin");
        }
    }
    SecretKey sk;
    from_file(context, sk, dir + "/sk.bin");
    RelinKeys rk;
    GaloisKeys gk;
    from_file(context, rk, dir + "/rk.bin");
    from_file(context, gk, dir + "/gk.bin");
    std::vector<Ciphertext> in(T);
    for (int t = 0; t < T; t++) from_file(context, in[t], dir + "/in" + std::to_string(t) + ".bin");
    const std::size_t L = in[0].coeff_modulus_size();
    check(L == 3, "inputs at three data primes");
    util::OpCombiner &comb = util::OpCombiner::instance();

    // ---- eight threads: each rotates its own ciphertext by its own step, squares and relinearizes ---------------------------
    auto work = [&](const Ciphertext &x, int t, const GaloisKeys &keys) {
        Ciphertext a, sq;
        evaluator.rotate_vector(x, (t % 4) + 1, keys, a);
        Words w = a.download();
        evaluator.square(a, sq);
        evaluator.relinearize_inplace(sq, rk);
        append(w, sq.download());
        return w;
    };
    std::vector<Words> want(T);
    for (int t = 0; t < T; t++) want[t] = work(in[t], t, gk);
    bool met = false;
    std::vector<Words> got(T);
    for (int round = 0; round < 20 && !met; round++)
    {
        util::RotationCache::instance().clear(); // the rotations must reach the combiner, not the cache
        got.assign(T, Words());
        moai_op_trace(1);
        {
            std::vector<std::thread> th;
            for (int t = 0; t < T; t++) th.emplace_back([&, t] { got[t] = work(in[t], t, gk); });
            for (auto &x : th) x.join();
        }
        moai_op_trace(0);
        for (int t = 0; t < T; t++) check(got[t] == want[t], "a thread's result equals the single-threaded one");
        // every rotation and every relinearization is in the census once, however they were grouped
        check(traced("apply_galois_to", L) == (unsigned long long)T && traced("relinearize", L) == (unsigned long long)T, "census of one round");
        // rounds go on until callers have met in both kinds of group.  Two threads share each step, so by default a rotation group
        // has at most two members; under the knob four different steps are in flight and a group of more than two mixes steps.
        // Relinearizations all use one key: their groups go through moai_relinearize_ptrs.
        met = !combining || (comb.largest_group(0) > (any_key ? 2u : 1u) && comb.largest_group(1) > 1u);
    }
    std::printf("largest groups: rotations %zu, relinearizations %zu\n", comb.largest_group(0), comb.largest_group(1));
    if (combining) check(met, "concurrent rotations and relinearizations shared calls (under the knob: rotations by different steps)");
    if (combining && !any_key) check(comb.largest_group(0) <= 2, "by default only rotations by the same step share a call");
    if (!combining) check(comb.largest_group(0) == 0 && comb.largest_group(1) == 0, "MOAI_SHIM_COMBINE_US=0: nothing goes through the combiner");
    {
        // what the threads of the last round computed, grouped as this setting groups them
        Words all;
        for (int t = 0; t < T; t++) append(all, got[t]);
        std::ofstream f(dir + "/out_" + tag + ".bin", std::ios::binary);
        f.write(reinterpret_cast<const char *>(all.data()), (std::streamsize)(all.size() * 8));
    }

    // ---- one thread, four pending rotations of four sources by four steps -----------------------------------------------------
    {
        std::vector<Words> single(4), src(4);
        for (int i = 0; i < 4; i++)
        {
            src[i] = in[i].download();
            Ciphertext r;
            evaluator.rotate_vector(in[i], i + 1, gk, r);
            single[i] = r.download(); // read at once: made alone
        }
        util::RotationCache::instance().clear();
        std::vector<Ciphertext> r(4);
        for (int i = 0; i < 4; i++) evaluator.rotate_vector(in[i], i + 1, gk, r[i]);
        moai_op_trace(1);
        const Words first = r[0].download();
        moai_op_trace(0);
        const unsigned long long made = traced("apply_galois_to", L);
        std::printf("pending rotations made by the first read: %llu\n", made);
        // the census sums the batch arguments: 4 after ONE read is one call of batch 4 (the other three were not asked for yet)
        check(made == (any_key ? 4u : 1u), "reading one of four pending rotations by different steps");
        check(first == single[0], "pending rotation 0");
        for (int i = 1; i < 4; i++) check(r[i].download() == single[i], "pending rotation i");
        for (int i = 0; i < 4; i++) check(in[i].download() == src[i], "sources intact");
    }

    // ---- a born-limited key asked above its limit, beside members whose keys serve the level -------------------------------
    {
        KeyGenerator gen(context, sk);
        GaloisKeys lim;
        // chain index 2 = the whole key; step 3's key is limited to chain index 0 (one data prime)
        moai_fused::create_galois_keys_limited(gen, elts, { 2, 2, 0, 2 }, lim);
        check(lim.born_limited(GaloisKeys::get_index(elts[2])) && !lim.born_limited(GaloisKeys::get_index(elts[0])), "one limited key in the set");
        std::vector<Words> ref(T), before(T);
        for (int t = 0; t < T; t++)
        {
            before[t] = in[t].download();
            if (t % 4 != 2) ref[t] = work(in[t], t, lim);
        }
        for (int round = 0; round < 3; round++)
        {
            util::RotationCache::instance().clear();
            std::vector<Words> got(T);
            std::vector<int> threw(T, 0);
            std::vector<std::thread> th;
            for (int t = 0; t < T; t++)
            {
                th.emplace_back([&, t] {
                    try { got[t] = work(in[t], t, lim); }
                    catch (const std::logic_error &) { threw[t] = 1; }
                    catch (...) { threw[t] = 2; }
                });
            }
            for (auto &x : th) x.join();
            for (int t = 0; t < T; t++)
            {
                check(threw[t] == (t % 4 == 2 ? 1 : 0), "only the member above its key's limit throws, and it throws std::logic_error");
                if (t % 4 != 2) check(got[t] == ref[t], "the other members of the round get their results");
                check(in[t].download() == before[t], "every member's operand is intact");
            }
        }
    }
    unsigned long long checked = 0, violations = 0;
    moai_debug_stream_audit_counts(&checked, &violations);
    std::printf("bad %d violations %llu checked %llu\n", bad, violations, checked);
    return bad ? 1 : 0;
}
"""

CAP_PROGRAM = r"""
#include <atomic>
#include <cstdio>
#include <thread>
#include "seal/moai_combiner.h"
using namespace seal::util;
int main()
{
    const int T = 80, CAP = 8;
    OpCombiner comb(20000, CAP); // a window of 20 ms, groups of at most 8
    if (comb.max_batch() != (std::size_t)CAP || OpCombiner::instance().max_batch() != 64) { std::printf("FAIL max_batch\n"); return 1; }
    std::vector<std::atomic<int>> served(T);
    for (auto &s : served) s.store(0);
    std::mutex mu;
    std::size_t largest = 0, groups = 0;
    int rounds = 0;
    const OpCombiner::Key key(0, 1, 0, nullptr, nullptr);
    // the first round teaches the combiner how many threads are calling; a later one fills groups to the cap
    for (; rounds < 10 && largest < (std::size_t)CAP; rounds++)
    {
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++)
        {
            th.emplace_back([&, t] {
                OpCombiner::Request r{ reinterpret_cast<const std::uint64_t *>((std::uintptr_t)(t + 1)), nullptr };
                comb.submit(key, r, [&](const std::vector<OpCombiner::Request> &reqs) {
                    std::lock_guard<std::mutex> g(mu); // the stub leader: notes the group and serves its members
                    largest = reqs.size() > largest ? reqs.size() : largest;
                    groups++;
                    for (const auto &q : reqs) served[(std::size_t)reinterpret_cast<std::uintptr_t>(q.in) - 1]++;
                });
            });
        }
        for (auto &x : th) x.join();
        for (int t = 0; t < T; t++)
        {
            if (served[t].load() != rounds + 1) { std::printf("FAIL request %d served %d times after %d rounds\n", t, served[t].load(), rounds + 1); return 1; }
        }
        if (largest > (std::size_t)CAP) { std::printf("FAIL a group of %zu exceeds the cap %d\n", largest, CAP); return 1; }
    }
    std::printf("rounds %d groups %zu largest %zu (combiner's own count %zu)\n", rounds, groups, largest, comb.largest_group(0));
    if (largest != (std::size_t)CAP || comb.largest_group(0) != largest) { std::printf("FAIL no group reached the cap\n"); return 1; }
    std::printf("cap ok\n");
    return 0;
}
"""


def _compile(tmp_path, text, name, link=True):
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    exe = tmp_path / name
    # g++ must be present: a missing compiler fails this test, it does not skip it
    cmd = ["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "seal_shim"), str(src),
           "-o", str(exe)]
    if link:
        cmd += ["-fopenmp", "-L" + PKG, "-lmoai_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, args, **env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("MOAI_SHIM_COMBINE") and k != "MOAI_STREAM_AUDIT"}
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(base, **env))
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.gpu
def test_shim_results_do_not_depend_on_the_grouping(tmp_path):
    exe = _compile(tmp_path, PROGRAM, "keyswitch_ptrs_shim")
    outs = {
        "off": _run(exe, ["setup", tmp_path, "off"], MOAI_SHIM_COMBINE_US="0"),
        "default": _run(exe, ["run", tmp_path, "default"]),
        "any": _run(exe, ["run", tmp_path, "any"], MOAI_SHIM_COMBINE_ANY_KEY="1"),
        "audit": _run(exe, ["run", tmp_path, "audit"], MOAI_SHIM_COMBINE_ANY_KEY="1", MOAI_STREAM_AUDIT="1"),
    }
    for tag, out in outs.items():
        assert "bad 0 violations 0" in out, (tag, out)
    assert " checked 0" not in outs["audit"].splitlines()[-1]  # the audit was live
    words = {tag: (tmp_path / ("out_%s.bin" % tag)).read_bytes() for tag in outs}
    # eight members, each a rotated [2][3][N] and a relinearized [2][3][N]
    assert len(words["off"]) == 8 * 2 * (2 * 3 * 4096) * 8
    for tag in ("default", "any", "audit"):
        assert words[tag] == words["off"], tag
    assert "pending rotations made by the first read: 1" in outs["default"]
    assert "pending rotations made by the first read: 4" in outs["any"]


def test_combiner_group_cap_host_only(tmp_path):
    """80 concurrent submitters on one combiner key, a stub in the leader's place: no group exceeds max_batch and every
    request is served exactly once (no device, no library)"""
    exe = _compile(tmp_path, CAP_PROGRAM, "combiner_cap", link=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "cap ok" in r.stdout, (r.stdout, r.stderr[-2000:])
