"""CKKSEncoder::decode_internal with sparse_slots_ != slots_ (SEAL/ckks.h:703-713, :757-760) restated on top of the
full-slot comparator tests/seal_decode.py, as the comparator of moai_ckks_decode_sparse (tests/test_oracle_decoder_sparse.py
pins it):

1. the inverse NTT and the exact CRT composition of seal_decode;
2. the projection onto the sparse subring: every composed coefficient i with i mod (N/2 / sparse_slots) != 0 becomes 0
   (the reference zeroes all its words: ((i - 1) & (sparsity - 1)) != sparsity - 1);
3. the word-by-word conversion, the forward DWT and the gather of seal_decode, of which the first sparse_slots entries
   are returned.
CPU only."""
import numpy as np

import seal_decode as SD


def project(x, sparse_slots):
    """step 2 on the composed integers x (object array [N])."""
    n = x.shape[0]
    sparsity = (n // 2) // int(sparse_slots)
    out = x.copy()
    keep = (np.arange(n) % sparsity) == 0
    out[~keep] = 0
    return out


def decode(octx, enc, plain_ntt, L, scale, sparse_slots, prime_index=None, is_complex=False):
    """plain_ntt [L][N] NTT form under primes prime_index (None = 0..L-1) -> the reference's sparse_slots decoded slots."""
    idx = list(range(L)) if prime_index is None else [int(i) for i in prime_index]
    primes = [octx.primes[i] for i in idx]
    coeff = octx.ntt(np.asarray(plain_ntt, dtype=np.uint64).reshape(1, L, -1), L, prime_index=prime_index,
                     inverse=True).reshape(L, -1)
    x = project(SD.compose(coeff, primes), sparse_slots)
    out = SD.decode_coeffs(enc, SD.convert(x, primes, scale), is_complex=True)[: int(sparse_slots)]
    return out if is_complex else np.ascontiguousarray(out.real)
