// The arithmetic of the passes that finish a 60-bit transform (csrc/ntt_finish.h: N^-1 by shift, the one-step final reduction)
// against unsigned __int128 arithmetic.  Host only, no library: the helpers are the same text the kernels compile.
//   logn 12, 13, 16; primes = 1 (mod 2N): the largest below 2^60, the smallest above 2^59, the largest of 52 bits, the smallest
//   above 2^20; inputs 0, 1, N - 1, N, q - 1, q, every multiple of q below the bound, the bound - 1, - (N - 1), - N, and 10^5
//   random values below the bound (16q for both helpers).
// Asserted per input: the residue, that no intermediate exceeds 64 bits (every step is redone in 128 bits and compared), and the
// output bound the call sites rely on (below 2q: one conditional subtraction to the canonical residue).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ntt_finish.h"

typedef unsigned __int128 u128;

static int g_fail = 0;
#define CHECK(cond, ...)                      \
    do                                        \
    {                                         \
        if (!(cond))                          \
        {                                     \
            if (g_fail < 20)                  \
            {                                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
            ++g_fail;                         \
        }                                     \
    } while (0)

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q)
{
    return (uint64_t)((u128)a * b % q);
}
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q)
{
    uint64_t r = 1;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
    {
        if (e & 1)
        {
            r = mulmod(r, a, q);
        }
    }
    return r;
}
// Miller-Rabin with the bases that decide every n < 2^64
static bool is_prime(uint64_t n)
{
    static const uint64_t small[] = { 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37 };
    if (n < 2)
    {
        return false;
    }
    for (uint64_t p : small)
    {
        if (n % p == 0)
        {
            return n == p;
        }
    }
    uint64_t d = n - 1;
    int s = 0;
    while (!(d & 1))
    {
        d >>= 1;
        ++s;
    }
    for (uint64_t a : small)
    {
        uint64_t x = powmod(a, d, n);
        if (x == 1 || x == n - 1)
        {
            continue;
        }
        bool comp = true;
        for (int i = 1; i < s && comp; ++i)
        {
            x = mulmod(x, x, n);
            comp = x != n - 1;
        }
        if (comp)
        {
            return false;
        }
    }
    return true;
}
// the first prime = 1 (mod 2N) at or beyond `start`, walking down (-1) or up (+1)
static uint64_t ntt_prime(int logn, uint64_t start, int dir)
{
    const uint64_t m = 2ull << logn;
    uint64_t q = dir < 0 ? start - (start - 1) % m : start + (m - (start - 1) % m) % m;
    while (!is_prime(q))
    {
        q = dir < 0 ? q - m : q + m;
    }
    return q;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static std::vector<uint64_t> inputs(uint64_t q, int logn, int bound_q)
{
    const uint64_t n = 1ull << logn, bound = (uint64_t)bound_q * q; // 16q < 2^64 for q < 2^60
    std::vector<uint64_t> v = { 0, 1, n - 1, n, q - 1, q, bound - 1, bound - (n - 1), bound - n };
    for (int k = 1; k < bound_q; ++k)
    {
        v.push_back((uint64_t)k * q);
    }
    for (int i = 0; i < 100000; ++i)
    {
        v.push_back((uint64_t)(((u128)rnd() * bound) >> 64));
    }
    return v;
}

static void check_ninv(uint64_t q, int logn)
{
    const uint64_t n = 1ull << logn, qh = moai::ninv_shift_qh(q, logn);
    CHECK(qh * n + 1 == q, "q = %llu is not 1 mod N", (unsigned long long)q);
    CHECK((qh >> 56) == 0, "the high word of qh exceeds 24 bits, q = %llu", (unsigned long long)q);
    const uint64_t ninv = powmod(n % q, q - 2, q);
    for (uint64_t x : inputs(q, logn, moai::NINV_SHIFT_IN))
    {
        const uint64_t got = moai::ninv_by_shift(x, qh, logn);
        // the same steps in 128 bits: nothing may exceed 64
        const u128 m = (u128)((0 - x) & (n - 1));
        const u128 xm = (u128)x + m, prod = m * qh, full = (xm >> logn) + prod;
        CHECK((xm >> 64) == 0 && (prod >> 64) == 0 && (full >> 64) == 0, "overflow at x = %llu, q = %llu", (unsigned long long)x, (unsigned long long)q);
        CHECK((uint64_t)(xm & (n - 1)) == 0, "x + m is no multiple of N at x = %llu", (unsigned long long)x);
        CHECK((u128)got == full, "64-bit result differs from the 128-bit one at x = %llu, q = %llu", (unsigned long long)x, (unsigned long long)q);
        CHECK(got % q == mulmod(x % q, ninv, q), "residue at x = %llu, q = %llu, logn = %d", (unsigned long long)x, (unsigned long long)q, logn);
        // the call site (inv_strided_tile): one conditional subtraction
        CHECK((u128)got < (u128)moai::NINV_SHIFT_OUT * q, "bound at x = %llu, q = %llu, logn = %d: %llu", (unsigned long long)x, (unsigned long long)q,
              logn, (unsigned long long)got);
    }
}

static void check_final(uint64_t q, int logn)
{
    const uint32_t s = moai::final_step_shift(q), M = moai::final_step_mult(q, s);
    const u128 mfull = ((u128)1 << (32 + s)) / q;
    CHECK((mfull >> 32) == 0 && (u128)M == mfull, "M does not fit 32 bits, q = %llu", (unsigned long long)q);
    const uint64_t nq = 0 - q;
    for (uint64_t z : inputs(q, logn, moai::FINAL_STEP_IN))
    {
        CHECK((z >> s) < (1ull << 24), "z >> s = %llu at z = %llu, q = %llu", (unsigned long long)(z >> s), (unsigned long long)z, (unsigned long long)q);
        const uint64_t got = moai::final_quotient_step(z, s, M, nq);
        const u128 k = ((u128)(z >> s) * M) >> 32;
        CHECK(k * q <= (u128)z, "quotient estimate above z / q at z = %llu, q = %llu", (unsigned long long)z, (unsigned long long)q);
        const u128 full = (u128)z - k * q;
        CHECK(z / q - (uint64_t)k <= 1, "quotient estimate short by %llu at z = %llu, q = %llu", (unsigned long long)(z / q - (uint64_t)k),
              (unsigned long long)z, (unsigned long long)q);
        CHECK((u128)got == full, "64-bit result differs from the 128-bit one at z = %llu, q = %llu", (unsigned long long)z, (unsigned long long)q);
        CHECK(got % q == z % q, "residue at z = %llu, q = %llu", (unsigned long long)z, (unsigned long long)q);
        CHECK((u128)got < (u128)moai::FINAL_STEP_OUT * q, "bound at z = %llu, q = %llu", (unsigned long long)z, (unsigned long long)q);
        // the call site (lazy_final): one conditional subtraction gives the canonical residue
        CHECK((got >= q ? got - q : got) == z % q, "canonical residue at z = %llu, q = %llu", (unsigned long long)z, (unsigned long long)q);
    }
}

int main()
{
    CHECK(moai::pack64(0x89abcdefu, 0x01234567u) == 0x0123456789abcdefull, "pack64");
    for (int logn : { 12, 13, 16 })
    {
        const uint64_t primes[] = { ntt_prime(logn, (1ull << 60) - 1, -1), ntt_prime(logn, (1ull << 59) + 1, +1),
                                    ntt_prime(logn, (1ull << 52) - 1, -1), ntt_prime(logn, (1ull << 20) + 1, +1) };
        CHECK(primes[0] < (1ull << 60) && primes[1] > (1ull << 59) && (primes[2] >> 51) == 1 && primes[3] > (1ull << 20) && primes[3] < (1ull << 24),
              "prime search, logn = %d", logn);
        for (uint64_t q : primes)
        {
            CHECK((q - 1) % (2ull << logn) == 0 && is_prime(q), "q = %llu", (unsigned long long)q);
            check_ninv(q, logn);
            check_final(q, logn);
            std::printf("logn %2d q %20llu (s = %2u, M = %10u): %s\n", logn, (unsigned long long)q, moai::final_step_shift(q),
                        moai::final_step_mult(q, moai::final_step_shift(q)), g_fail ? "FAIL" : "ok");
        }
    }
    if (g_fail)
    {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ALL PASS\n");
    return 0;
}
