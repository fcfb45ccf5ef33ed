// Host-only: the sparse-slot diagonal sets of bootstrapping/moai_fft_diagonals.h against the definition, for logNh = 10 and
// every supported logn < 10, the way tests/cpp/test_bootstrap_setup.cpp checks the full-slot sets.  The sets act on
// 2n-periodic slot vectors exactly as BsgsLinearTransform applies them (diagonals replicated, rotations by true offsets).
//   forward: slottocoeff_3 without the runtime scale -- the three centred sets, then x + rotate(x, n) -- maps the real vector
//            (a, b) of 2n entries to U P (a + i b) in every n-block (U[j][k] = zeta^(5^j k), zeta = exp(2 pi i / 4n),
//            P the bit reversal of n points), checked against the O(n^2) sum;
//   inverse: the three coefficient-to-slot sets on F(a, b) give (a + i b) / (2 K 2^(logNh - logn)) in the first n slots and
//            -i times that in the second n; the conjugate-and-add of coefftoslot_3 then gives (a, b) / (K 2^(logNh - logn)).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>

#include "moai_fft_diagonals.h"

using cplx = std::complex<double>;
using Set = std::vector<std::vector<cplx>>;
static int g_checks = 0, g_fail = 0;
#define CHECK(cond)                                                \
    do                                                             \
    {                                                              \
        g_checks++;                                                \
        if (!(cond))                                               \
        {                                                          \
            g_fail++;                                              \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                          \
    } while (0)

// y[s] = sum_i D_i[s mod len] x[(s + off_i) mod M]
static std::vector<cplx> apply(const Set &D, int totlen, int basicstep, bool rotated, const std::vector<cplx> &x)
{
    const int M = static_cast<int>(x.size());
    std::vector<cplx> y(M, 0.0);
    for (std::size_t i = 0; i < D.size(); i++)
    {
        const int off = rotated ? static_cast<int>(i) * basicstep : (static_cast<int>(i) - totlen) * basicstep;
        const int len = static_cast<int>(D[i].size());
        for (int s = 0; s < M; s++)
        {
            y[s] += D[i][s % len] * x[((s + off) % M + M) % M];
        }
    }
    return y;
}

static int bitrev(int v, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; b++)
    {
        r |= ((v >> b) & 1) << (bits - 1 - b);
    }
    return r;
}

int main()
{
    const int logNh = 10;
    const long K = 25;
    for (int logn = 0; logn < logNh; logn++)
    {
        if (logn < 3)
        {
            bool threw = false;
            try
            {
                moai_boot::level_three_sparse_diagonals(logn, logNh, K);
            }
            catch (const std::invalid_argument &e)
            {
                threw = strstr(e.what(), logn == 0 ? "logn == 0" : "0 bits") != nullptr;
            }
            CHECK(threw);
            continue;
        }
        const int n = 1 << logn;
        const auto d = moai_boot::level_three_sparse_diagonals(logn, logNh, K);
        const auto f = moai_boot::forward_split(logn), v = moai_boot::inverse_split(logn);
        // shapes (the reference's sparse branch)
        CHECK(d.fftcoeff1.size() == static_cast<std::size_t>(2 * f.totlen[0] + 1) && d.fftcoeff1[0].size() == static_cast<std::size_t>(2 * n));
        CHECK(d.fftcoeff2.size() == static_cast<std::size_t>(2 * f.totlen[1] + 1) && d.fftcoeff2[0].size() == static_cast<std::size_t>(2 * n));
        CHECK(d.fftcoeff3.size() == static_cast<std::size_t>(2 * f.totlen[2] + 1) && d.fftcoeff3[0].size() == static_cast<std::size_t>(2 * n));
        CHECK(d.invfftcoeff1.size() == static_cast<std::size_t>(v.totlen[0] + 1) && d.invfftcoeff1[0].size() == static_cast<std::size_t>(n));
        CHECK(d.invfftcoeff2.size() == static_cast<std::size_t>(2 * v.totlen[1] + 1) && d.invfftcoeff2[0].size() == static_cast<std::size_t>(n));
        CHECK(d.invfftcoeff3.size() == static_cast<std::size_t>(2 * v.totlen[2] + 1) && d.invfftcoeff3[0].size() == static_cast<std::size_t>(2 * n));

        std::mt19937_64 rng(logn);
        std::uniform_real_distribution<double> ud(-1.0, 1.0);
        std::vector<double> a(n), b(n);
        for (int k = 0; k < n; k++)
        {
            a[k] = ud(rng);
            b[k] = ud(rng);
        }
        // forward on the 2n-periodic real vector (a, b), in a vector of M = 4n slots (two periods)
        const int M = 4 * n;
        std::vector<cplx> x(M);
        for (int s = 0; s < M; s++)
        {
            x[s] = (s % (2 * n)) < n ? a[s % n] : b[s % n];
        }
        auto y = apply(d.fftcoeff1, f.totlen[0], f.basicstep[0], false, x);
        y = apply(d.fftcoeff2, f.totlen[1], f.basicstep[1], false, y);
        y = apply(d.fftcoeff3, f.totlen[2], f.basicstep[2], false, y);
        std::vector<cplx> fw(M);
        for (int s = 0; s < M; s++)
        {
            fw[s] = y[s] + y[(s + n) % M];
        }
        double ferr = 0, fmax = 0;
        for (int j = 0; j < n; j++)
        {
            cplx want = 0;
            long pw = 1;
            for (int i = 0; i < j; i++)
            {
                pw = (pw * 5) % (4 * n);
            }
            for (int k = 0; k < n; k++)
            {
                const int pk = bitrev(k, logn);
                want += std::polar(1.0, 2 * M_PI * static_cast<double>((pw * k) % (4 * n)) / (4 * n)) * cplx(a[pk], b[pk]);
            }
            for (int r = 0; r < M / n; r++)
            {
                ferr = std::max(ferr, std::abs(fw[j + r * n] - want));
            }
            fmax = std::max(fmax, std::abs(want));
        }
        // inverse on the n-periodic F(a, b)
        auto z = apply(d.invfftcoeff1, v.totlen[0], v.basicstep[0], true, fw);
        z = apply(d.invfftcoeff2, v.totlen[1], v.basicstep[1], false, z);
        z = apply(d.invfftcoeff3, v.totlen[2], v.basicstep[2], false, z);
        const double c = 1.0 / (2.0 * K * (1 << (logNh - logn)));
        double ierr = 0, cerr = 0;
        for (int s = 0; s < M; s++)
        {
            const int k = s % n;
            const cplx t(a[k], b[k]);
            const cplx want = (s % (2 * n)) < n ? c * t : cplx(0, -1) * c * t;
            ierr = std::max(ierr, std::abs(z[s] - want));
            // coefftoslot_3: z + conj(z) gives 2 c (a, b)
            const double real_want = (s % (2 * n)) < n ? 2 * c * a[k] : 2 * c * b[k];
            cerr = std::max(cerr, std::abs(z[s] + std::conj(z[s]) - real_want));
        }
        printf("logn %d (split %d+%d+%d): forward max |error| %.2e (|U P t| <= %.1f), inverse %.2e, conjugate-add %.2e\n", logn,
               f.part[0], f.part[1], f.part[2], ferr, fmax, ierr, cerr);
        // the tolerances of tests/cpp/test_bootstrap_setup.cpp (forward 1e-9 n, G F relative to its factor 1e-11 n)
        CHECK(ferr < 1e-9 * n);
        CHECK(ierr / c < 1e-11 * n);
        CHECK(cerr / c < 1e-11 * n);
    }
    printf("%d checks, %d failed\n", g_checks, g_fail);
    if (!g_fail)
    {
        printf("ALL OK\n");
    }
    return g_fail ? 1 : 0;
}
