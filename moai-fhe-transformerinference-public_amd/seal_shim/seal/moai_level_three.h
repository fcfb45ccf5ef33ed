// seal/moai_level_three.h -- what the three users of MOAI's "level-3" bootstrapping transforms must agree on: how the
// log2 n butterfly stages are split into three groups (the diagonals of bootstrapping/moai_fft_diagonals.h, the rotation-key
// list boot_rotation_steps_3 and the transforms of PackedBootstrapper3, seal/moai_bootstrap_eval.h), and the six diagonal
// sets that travel between them.  Host-only, no other header of the shim needed.
#pragma once
#include <cmath>
#include <complex>
#include <utility>
#include <vector>

namespace moai_boot
{
    using cplx = std::complex<double>;
    using DiagonalSet = std::vector<std::vector<cplx>>; // [diagonal][slot]

    // The six sets of one slot count in the reference's layout (Bootstrapper.h:43-46, fftcoeff1..3 and invfftcoeff1..3 of one
    // slot index): 2 totlen + 1 diagonals for a plain transform, totlen + 1 for a rotated one; which is which, and the
    // diagonal lengths, are listed in bootstrapping/moai_fft_diagonals.h for full and for sparse slots.
    struct LevelThreeDiagonals
    {
        DiagonalSet fftcoeff1, fftcoeff2, fftcoeff3;          // slot-to-coefficient, applied 1, 2, 3
        DiagonalSet invfftcoeff1, invfftcoeff2, invfftcoeff3; // coefficient-to-slot, applied 1, 2, 3
    };

    struct LevelThreeSplit
    {
        int part[3]; // stages per group, in order of application
        int totlen[3];
        int basicstep[3];
    };
    // geninvfftcoeff_3's split (Bootstrapper.cpp:1567-1578; sflinv_full_3 :2603-2613, sflinv_3 :2580-2590,
    // addLeftRotKeys_Linear_to_vector_3 :89-184): the FIRST group gets floor(logn / 3) stages
    inline LevelThreeSplit inverse_split(int logn)
    {
        LevelThreeSplit s;
        s.part[0] = static_cast<int>(std::floor(logn / 3.0));
        s.part[1] = static_cast<int>(std::floor((logn - s.part[0]) / 2.0));
        s.part[2] = logn - s.part[0] - s.part[1];
        s.basicstep[0] = 1 << (logn - s.part[0]);
        s.basicstep[1] = 1 << (logn - s.part[0] - s.part[1]);
        s.basicstep[2] = 1;
        for (int i = 0; i < 3; i++)
        {
            s.totlen[i] = (1 << s.part[i]) - 1;
        }
        return s;
    }
    // genfftcoeff_3's split (:1159-1170; sfl_full_3 :2461-2471, sfl_3 :2420-2430): the LAST group gets floor(logn / 3)
    // stages -- the inverse's groups in the opposite order
    inline LevelThreeSplit forward_split(int logn)
    {
        LevelThreeSplit s = inverse_split(logn);
        std::swap(s.part[0], s.part[2]);
        std::swap(s.totlen[0], s.totlen[2]);
        std::swap(s.basicstep[0], s.basicstep[2]);
        return s;
    }
} // namespace moai_boot
