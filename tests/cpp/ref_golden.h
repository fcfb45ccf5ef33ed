// tests/cpp/ref_golden.h -- the bootstrapping tests' comparison with the reference, without the reference.
//
// test_bootstrap_lt / _eval / _real check the fused device pipeline bit for bit against the reference's own call sequence
// (tests/cpp/ref_bootstrapper.h).  That comparator is the reference's source text, which only a build next to the reference
// checkout has (oracle/Makefile, target ref_bootstrap).  So the tests run with fixed client randomness, and every compared
// ciphertext is reduced to a 64-bit digest of its level, scale and residues:
//   - built with MOAI_REF_SLICES (oracle/_ref/): the reference's sequence runs, the fused result is compared with it
//     directly, and the reference's digest is printed as "GOLDEN <name> <digest>";
//   - built in the tree (tests/cpp/Makefile): the fused result's digest is compared with the recorded one,
//     tests/golden/bootstrap_ref_digests.txt (those GOLDEN lines, collected on an MI355X).
#pragma once
#include <omp.h>
#include <unistd.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "seal/seal.h"

namespace refgolden
{
    // One ChaCha20 stream seeded with `seed` on the calling thread; the key generator's OpenMP loops (sample_uniform) are
    // kept on that thread until release(), so keys and encryptions are the same in every run.  Cost: one host thread draws
    // the keys, which at N = 2^16 (test_bootstrap_real --full: 47 Galois keys on the 36-prime chain) takes about 70 s of
    // the test's 900 s limit.
    class FixedRandomness
    {
    public:
        explicit FixedRandomness(std::uint64_t seed) : saved_(omp_get_max_threads())
        {
            unsigned char s[40] = { 0 };
            std::memcpy(s, &seed, sizeof(seed));
            std::memcpy(s + 32, "refgold", 8);
            seal::util::thread_rng() = seal::util::ChaCha20Rng(s);
            omp_set_num_threads(1);
        }
        // after key generation: encryption draws on the calling thread only
        void release()
        {
            omp_set_num_threads(saved_);
        }
        ~FixedRandomness()
        {
            release();
        }

    private:
        int saved_;
    };

    // FNV-1a over chain index, scale bits, size and residues
    inline std::uint64_t digest(const seal::SEALContext &context, const seal::Ciphertext &ct)
    {
        std::uint64_t h = 0xcbf29ce484222325ull;
        auto mix = [&](std::uint64_t w) {
            for (int i = 0; i < 8; i++)
            {
                h ^= (w >> (8 * i)) & 0xff;
                h *= 0x100000001b3ull;
            }
        };
        mix(context.get_context_data(ct.parms_id())->chain_index());
        double sc = ct.scale();
        std::uint64_t sb;
        std::memcpy(&sb, &sc, sizeof(sb));
        mix(sb);
        mix(ct.size());
        const std::vector<std::uint64_t> words = ct.download();
        mix(words.size());
        for (std::uint64_t w : words) mix(w);
        return h;
    }

    // tests/golden/bootstrap_ref_digests.txt, found from the binary's own location (tests/cpp/<binary>)
    inline const std::map<std::string, std::uint64_t> &recorded()
    {
        static const std::map<std::string, std::uint64_t> table = [] {
            std::map<std::string, std::uint64_t> t;
            char exe[PATH_MAX] = { 0 };
            const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
            std::string dir = n > 0 ? std::string(exe, (size_t)n) : std::string("./x");
            dir = dir.substr(0, dir.rfind('/'));
            std::ifstream f(dir + "/../golden/bootstrap_ref_digests.txt");
            if (!f)
            {
                std::printf("recorded digests not found: %s/../golden/bootstrap_ref_digests.txt\n", dir.c_str());
            }
            std::string line;
            while (std::getline(f, line))
            {
                if (line.empty() || line[0] == '#') continue;
                std::istringstream ss(line);
                std::string name, hex;
                if (ss >> name >> hex) t[name] = std::stoull(hex, nullptr, 16);
            }
            return t;
        }();
        return table;
    }

    inline void print_golden(const char *name, std::uint64_t d)
    {
        std::printf("GOLDEN %s %016llx\n", name, (unsigned long long)d);
    }

    // the fused result against the reference's recorded digest of the same computation
    inline bool matches_recorded(const std::string &name, const seal::SEALContext &context, const seal::Ciphertext &got)
    {
        const auto &t = recorded();
        const auto it = t.find(name);
        if (it == t.end())
        {
            std::printf("no recorded digest for %s\n", name.c_str());
            return false;
        }
        const std::uint64_t d = digest(context, got);
        if (d != it->second)
        {
            std::printf("%s: digest %016llx, the reference's %016llx\n", name.c_str(), (unsigned long long)d, (unsigned long long)it->second);
        }
        return d == it->second;
    }
} // namespace refgolden
