#!/usr/bin/env python3
"""The client's input path at MOAI's parameters (N = 2^16, the 36-prime chain), host against device in ONE process on the same
box: (1) Encryptor::encrypt of 768 plaintexts at the top data level against moai_fused::encrypt; (2) a MOAI-style loop
(encode + encrypt per column under OpenMP, Batch_encode_encrypt.hpp:8-38) against moai_fused::batch_input for 128 x 128 x 768
inputs; (3) KeyGenerator's relin key + the 31 power-of-two Galois keys against moai_fused::create_relin_keys /
create_galois_keys.  Compiles a small driver with g++ against the seal:: shim, runs it and prints one JSON line (seconds, and
the speed-ups).  OpenMP threads: OMP_NUM_THREADS, else 16."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moai-fhe-transformerinference-public_amd")

DRIVER = r"""
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
#include "seal/seal.h"
#include "seal/moai_fused.h"
using namespace seal;
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int main()
{
    const std::size_t n = 1 << 16;
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    std::vector<int> bits(1, 51);
    for (int i = 0; i < 20; i++) bits.push_back(46);
    for (int i = 0; i < 14; i++) bits.push_back(51);
    bits.push_back(58);
    parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
    SEALContext context(parms, true, sec_level_type::none);
    KeyGenerator keygen(context);
    CKKSEncoder encoder(context);
    const std::size_t slots = encoder.slot_count();
    const double scale = std::pow(2.0, 46);
    double t;
    // (3) keys
    double key_host, key_dev;
    {
        RelinKeys rk;
        GaloisKeys gk;
        t = now_s();
        keygen.create_relin_keys(rk);
        keygen.create_galois_keys(gk);
        key_host = now_s() - t;
    }
    {
        RelinKeys rk;
        GaloisKeys gk;
        t = now_s();
        moai_fused::create_relin_keys(keygen, rk);
        moai_fused::create_galois_keys(keygen, gk);
        context.sync();
        key_dev = now_s() - t;
        std::fprintf(stderr, "galois keys %zu\n", gk.size());
    }
    PublicKey pk;
    keygen.create_public_key(pk);
    Encryptor encryptor(context, pk);
    // (1) 768 encryptions at the top data level
    const int C = 768;
    std::vector<Plaintext> plains(C);
    {
        std::vector<double> v(slots);
        for (int i = 0; i < C; i++)
        {
            for (std::size_t j = 0; j < slots; j++) v[j] = std::sin(0.001 * (i + j));
            encoder.encode(v, scale, plains[i]);
        }
        context.sync();
    }
    double enc_host, enc_dev;
    {
        std::vector<Ciphertext> cts(C);
        t = now_s();
#pragma omp parallel for
        for (int i = 0; i < C; i++) encryptor.encrypt(plains[i], cts[i]);
        context.sync();
        enc_host = now_s() - t;
    }
    {
        std::vector<Ciphertext> cts;
        t = now_s();
        moai_fused::encrypt(encryptor, plains, cts);
        context.sync();
        enc_dev = now_s() - t;
    }
    plains.clear();
    // (2) batch_input
    const int num_X = 128, num_row = 128, num_col = 768;
    std::vector<std::vector<std::vector<double>>> X(num_X, std::vector<std::vector<double>>(num_row, std::vector<double>(num_col)));
    for (int j = 0; j < num_X; j++) for (int k = 0; k < num_row; k++) for (int i = 0; i < num_col; i++) X[j][k][i] = std::cos(0.01 * (j + k + i));
    double bi_host, bi_dev;
    {
        std::vector<Ciphertext> out(num_col);
        t = now_s();
#pragma omp parallel for
        for (int i = 0; i < num_col; ++i)
        {
            std::vector<double> vec(slots, 0);
            for (int j = 0; j < num_X; ++j) for (int k = 0; k < num_row; ++k) vec[num_X * k + j] = X[j][k][i];
            Plaintext p;
            encoder.encode(vec, scale, p);
            encryptor.encrypt(p, out[i]);
        }
        context.sync();
        bi_host = now_s() - t;
    }
    {
        t = now_s();
        auto out = moai_fused::batch_input(X, num_X, num_row, num_col, scale, context, pk);
        context.sync();
        bi_dev = now_s() - t;
    }
    std::printf("{\"encrypt_768_host_s\": %.4f, \"encrypt_768_device_s\": %.4f, \"batch_input_moai_loop_s\": %.4f, "
                "\"batch_input_device_s\": %.4f, \"relin_31_galois_host_s\": %.4f, \"relin_31_galois_device_s\": %.4f}\n",
                enc_host, enc_dev, bi_host, bi_dev, key_host, key_dev);
    return 0;
}
"""


def main():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "client_time.cpp"), os.path.join(d, "client_time")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(PKG, "seal_shim"), src, "-o", exe, "-L" + PKG, "-lmoai_hip",
                               "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
        env = dict(os.environ)
        env.setdefault("OMP_NUM_THREADS", "16")
        r = subprocess.run([exe], capture_output=True, text=True, env=env)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            return r.returncode
        res = json.loads(r.stdout.strip().splitlines()[-1])
        res["speedup_encrypt"] = round(res["encrypt_768_host_s"] / res["encrypt_768_device_s"], 1)
        res["speedup_batch_input"] = round(res["batch_input_moai_loop_s"] / res["batch_input_device_s"], 1)
        res["speedup_keys"] = round(res["relin_31_galois_host_s"] / res["relin_31_galois_device_s"], 1)
        print(json.dumps(res))
        return 0


if __name__ == "__main__":
    sys.exit(main())
