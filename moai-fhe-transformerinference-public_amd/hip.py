"""ctypes binding of libmoai_hip.so -- the C ABI declared in include/moai_hip.h.

This is plumbing, not product logic: every call goes straight to the HIP library.  Residue data is
numpy uint64 on the host and raw device pointers on the GPU, in the reference's layout
[poly][rns prime][coefficient] (SEAL/ciphertext.h:337-349).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libmoai_hip.so")

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
vp = C.c_void_p
sz = C.c_size_t

# name -> (restype, argtypes); must list every symbol include/moai_hip.h declares
SYMBOLS = {
    "moai_last_error": (C.c_char_p, []),
    "moai_version": (C.c_int, []),
    "moai_ctx_create": (C.c_int, [C.c_int, u64p, sz, C.c_int, C.POINTER(vp)]),
    "moai_ctx_destroy": (None, [vp]),
    "moai_ctx_reserve": (C.c_int, [vp, sz]),
    "moai_ctx_reserve_stream": (C.c_int, [vp, vp, sz]),
    "moai_ctx_coeff_count": (sz, [vp]),
    "moai_ctx_prime_count": (sz, [vp]),
    "moai_ctx_root": (C.c_uint64, [vp, sz]),
    "moai_ctx_prime": (C.c_uint64, [vp, sz]),
    "moai_malloc": (C.c_int, [C.POINTER(vp), sz]),
    "moai_free": (C.c_int, [vp]),
    "moai_memcpy_h2d": (C.c_int, [vp, vp, sz, vp]),
    "moai_memcpy_d2h": (C.c_int, [vp, vp, sz, vp]),
    "moai_memcpy_d2d": (C.c_int, [vp, vp, sz, vp]),
    "moai_memset_zero": (C.c_int, [vp, sz, vp]),
    "moai_stream_create": (C.c_int, [C.POINTER(vp)]),
    "moai_stream_destroy": (C.c_int, [vp]),
    "moai_stream_sync": (C.c_int, [vp]),
    "moai_ntt_forward": (C.c_int, [vp, vp, sz, sz, u32p, vp]),
    "moai_ntt_inverse": (C.c_int, [vp, vp, sz, sz, u32p, vp]),
    "moai_add": (C.c_int, [vp, vp, vp, vp, sz, sz, vp]),
    "moai_sub": (C.c_int, [vp, vp, vp, vp, sz, sz, vp]),
    "moai_negate": (C.c_int, [vp, vp, vp, sz, sz, vp]),
    "moai_dyadic_mul": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_mul_scalar_rows": (C.c_int, [vp, vp, u64p, vp, sz, sz, vp]),
    "moai_add_scalar_rows": (C.c_int, [vp, vp, u64p, vp, sz, sz, vp]),
    "moai_mul_i_add": (C.c_int, [vp, vp, vp, vp, sz, sz, C.c_int, vp]),
    "moai_real_split": (C.c_int, [vp, vp, vp, vp, vp, sz, sz, vp]),
    "moai_ct_multiply": (C.c_int, [vp, vp, vp, vp, sz, sz, vp]),
    "moai_ct_square": (C.c_int, [vp, vp, vp, sz, sz, vp]),
    "moai_ct_multiply_general": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, sz, vp]),
    "moai_ct_dot": (C.c_int, [vp, vp, vp, vp, sz, sz, vp]),
    "moai_ct_pt_dot": (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), sz, sz, sz, vp]),
    "moai_ct_pt_dot_rows": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_ct_pt_dot2": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), sz, sz, sz, sz, vp]),
    "moai_ct_pt_matmul": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, sz, vp]),
    "moai_rescale": (C.c_int, [vp, vp, vp, sz, sz, sz, vp]),
    "moai_mul_scalar_rescale": (C.c_int, [vp, vp, u64p, vp, sz, sz, sz, vp]),
    "moai_rescale_add": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_mul_scalar_rescale_add": (C.c_int, [vp, vp, u64p, vp, vp, sz, sz, sz, vp]),
    "moai_mod_drop": (C.c_int, [vp, vp, vp, sz, sz, sz, sz, vp]),
    "moai_galois_permute": (C.c_int, [vp, vp, vp, sz, sz, C.c_uint32, vp]),
    "moai_galois_elt_from_step": (C.c_uint32, [vp, C.c_int]),
    "moai_switch_key": (C.c_int, [vp, vp, vp, vp, sz, sz, vp]),
    "moai_relinearize": (C.c_int, [vp, vp, vp, vp, sz, sz, vp]),
    "moai_apply_galois": (C.c_int, [vp, vp, sz, C.c_uint32, vp, sz, vp]),
    "moai_apply_galois_to": (C.c_int, [vp, vp, vp, sz, C.c_uint32, vp, sz, vp]),
    "moai_apply_galois_acc": (C.c_int, [vp, vp, vp, sz, C.c_uint32, vp, sz, vp]),
    "moai_modraise": (C.c_int, [vp, vp, vp, sz, sz, vp]),
    "moai_hoist_correction": (C.c_int, [vp, vp, C.c_uint32, sz, vp, vp]),
    "moai_apply_galois_hoisted": (C.c_int, [vp, vp, C.POINTER(vp), sz, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(vp), sz, sz, C.POINTER(C.c_int), vp]),
    "moai_ckks_encode": (C.c_int, [vp, vp, C.c_int, sz, sz, vp, sz, C.POINTER(C.c_uint32), C.c_double, vp, vp]),
    "moai_ckks_encode_masked": (C.c_int, [vp, vp, vp, sz, sz, vp, sz, C.POINTER(C.c_uint32), C.c_double, vp, vp]),
    "moai_decrypt": (C.c_int, [vp, vp, sz, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_ckks_decode": (C.c_int, [vp, vp, sz, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_int, vp, vp]),
    "moai_ckks_decode_sparse": (C.c_int, [vp, vp, sz, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_double), sz, C.c_int, vp, vp]),
    "moai_sample_uniform": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_sample_ternary": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_sample_cbd": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_encrypt_symmetric": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_encrypt_asymmetric": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, vp, vp, sz, sz, vp]),
    "moai_kswitch_keygen": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, vp, vp, vp]),
    "moai_packed_words": (sz, [vp, sz, C.POINTER(C.c_uint32)]),
    "moai_pack_rows": (C.c_int, [vp, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_unpack_rows": (C.c_int, [vp, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp, vp]),
    "moai_encrypt_symmetric_seeded": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_kswitch_keygen_seeded": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, vp, vp]),
    "moai_expand_seeded": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp]),
    "moai_seal_prng_bytes": (C.c_int, [vp, C.c_char_p, C.c_uint64, C.c_uint64, vp, vp]),
    "moai_seal_sample_uniform": (C.c_int, [vp, C.c_char_p, vp, sz, sz, sz, C.POINTER(C.c_uint32), vp, vp]),
    "moai_encrypt_symmetric_seal_seeded": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, vp, sz, sz, C.POINTER(C.c_uint32), vp, vp]),
    "moai_kswitch_keygen_seal_seeded": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, vp, vp, vp]),
    "moai_check_residues": (C.c_int, [vp, vp, sz, sz, C.POINTER(C.c_uint32), vp, vp]),
    "moai_total_coeff_modulus_bit_count": (C.c_int, [vp, sz, C.POINTER(C.c_uint32)]),
    "moai_ckks_tables": (C.c_int, [vp, vp, vp]),
    "moai_set_tuning": (C.c_int, [C.c_char_p, C.c_long]),
    "moai_reset_tuning": (C.c_int, []),
    "moai_ntt_pipe_plan": (sz, [sz, sz, sz, sz, C.c_long, C.c_long]),
    "moai_arith_mode": (C.c_int, [vp, sz, C.c_int, sz, sz, C.POINTER(C.c_int)]),
    "moai_mem_info": (C.c_int, [C.POINTER(sz), C.POINTER(sz)]),
    "moai_op_trace": (C.c_int, [C.c_int]),
    "moai_op_trace_dump": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "moai_scalar_dot": (C.c_int, [vp, C.POINTER(vp), u64p, sz, vp, vp, sz, sz, vp]),
    "moai_vector_dot": (C.c_int, [vp, C.POINTER(vp), vp, sz, vp, vp, sz, sz, vp]),
    "moai_ct_dot_ptrs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), sz, vp, vp, sz, vp]),
    "moai_apply_galois_ptrs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(vp), sz, vp]),
    "moai_relinearize_ptrs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), vp, sz, sz, vp]),
    "moai_hybrid_digits": (sz, [vp, sz, sz]),
    "moai_hybrid_keygen": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, vp, sz, vp, vp]),
    "moai_switch_key_hybrid": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_relinearize_hybrid": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_apply_galois_hybrid": (C.c_int, [vp, vp, sz, sz, C.c_uint32, vp, sz, vp]),
    "moai_hybrid_hoist_correction": (C.c_int, [vp, vp, C.c_uint32, sz, sz, vp, vp]),
    "moai_apply_galois_hybrid_hoisted": (C.c_int, [vp, vp, C.POINTER(vp), sz, sz, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(vp), sz, sz, C.POINTER(C.c_int), vp]),
    "moai_hybrid_rotate_pt_dot": (C.c_int, [vp, vp, C.POINTER(vp), sz, sz, sz, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(vp), sz, C.POINTER(C.c_int), vp]),
    "moai_hybrid_bsgs_dot": (C.c_int, [vp, vp, vp, sz, sz, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(C.c_uint32), C.POINTER(vp), sz, C.POINTER(vp), sz, C.POINTER(C.c_int), vp]),
    "moai_relinearize_rescale_hybrid": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_multiply_relin_rescale_hybrid": (C.c_int, [vp, vp, vp, vp, vp, sz, sz, sz, vp]),
    "moai_apply_galois_hybrid_to": (C.c_int, [vp, vp, vp, sz, sz, C.c_uint32, vp, sz, vp]),
    "moai_apply_galois_hybrid_acc": (C.c_int, [vp, vp, vp, sz, sz, C.c_uint32, vp, sz, vp]),
    "moai_apply_galois_hybrid_ptrs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), sz, sz, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(vp), sz, vp]),
    "moai_relinearize_hybrid_ptrs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), vp, sz, sz, sz, vp]),
    "moai_relinearize_rescale_hybrid_ptrs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), vp, sz, sz, sz, vp]),
    "moai_hybrid_set_rounding": (C.c_int, [vp, C.c_int]),
    "moai_hybrid_rounding": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "moai_gather_blocks": (C.c_int, [vp, C.POINTER(vp), vp, sz, sz, vp]),
    "moai_scatter_blocks": (C.c_int, [vp, vp, C.POINTER(vp), sz, sz, vp]),
    "moai_key_words": (sz, [vp, sz]),
    "moai_key_trim": (C.c_int, [vp, vp, sz, vp, vp]),
    "moai_key_forget": (C.c_int, [vp, vp]),
    "moai_kswitch_keygen_limited": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, vp, sz, vp, vp]),
    "moai_kswitch_keygen_limited_seeded": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_uint64, vp, vp, sz, vp, vp]),
    "moai_expand_seeded_limited": (C.c_int, [vp, C.c_char_p, C.c_uint64, vp, sz, vp, vp]),
    "moai_key_register": (C.c_int, [vp, vp, sz]),
    "moai_debug_stream_audit": (C.c_int, [C.c_int]),
    "moai_debug_block_label": (None, [vp, sz, vp, C.c_int]),
    "moai_debug_stream_audit_counts": (None, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "moai_device_info": (C.c_int, [C.c_int, C.c_char_p, sz, C.POINTER(C.c_int), C.POINTER(sz)]),
    "moai_event_create": (C.c_int, [C.POINTER(vp)]),
    "moai_event_destroy": (C.c_int, [vp]),
    "moai_event_record": (C.c_int, [vp, vp]),
    "moai_event_synchronize": (C.c_int, [vp]),
    "moai_host_malloc": (C.c_int, [C.POINTER(vp), sz]),
    "moai_host_free": (C.c_int, [vp]),
    "moai_event_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
}


MOAI_EINVAL = -1  # include/moai_hip.h
HYBRID_ROUND_FAST, HYBRID_ROUND_EXACT = 0, 1  # MOAI_HYBRID_ROUND_* of include/moai_hip.h
# moai_arith_mode: the arithmetic modes and the operations it answers for (include/moai_hip.h)
MODE_LAZY16, MODE_LAZY8, MODE_GUARD2, MODE_GUARD, MODE_NOGUARD, MODE_FPN, MODE_FPR = -3, -2, -1, 0, 1, 2, 3
MODE_OF_KEY_SWITCH, MODE_OF_MOD_DOWN, MODE_OF_NTT_FORWARD, MODE_OF_NTT_INVERSE = 0, 1, 2, 3


class MoaiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("moai_hip error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    return _SO


_lib = None


def lib():
    """Load libmoai_hip.so.  Raises (never falls back) when the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError(
                "%s is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')" % _SO
            )
        L = C.CDLL(_SO)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MoaiError(rc, lib().moai_last_error().decode())


class DeviceBuffer:
    """A block of device memory holding uint64 residues (moai_malloc / moai_free)."""

    def __init__(self, n_words):
        self.n_words = int(n_words)
        p = vp()
        _check(lib().moai_malloc(C.byref(p), self.n_words * 8))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a, stream=None):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = cls(a.size)
        b.upload(a, stream)
        return b

    def upload(self, a, stream=None):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        assert a.size <= self.n_words
        _check(lib().moai_memcpy_h2d(self.ptr, a.ctypes.data, a.size * 8, stream))
        _check(lib().moai_stream_sync(stream))

    def to_numpy(self, shape=None, stream=None, words=None):
        words = self.n_words if words is None else words
        out = np.empty(words, dtype=np.uint64)
        _check(lib().moai_stream_sync(stream))
        _check(lib().moai_memcpy_d2h(out.ctypes.data, self.ptr, words * 8, stream))
        _check(lib().moai_stream_sync(stream))
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr:
            lib().moai_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KeyBuffer(DeviceBuffer):
    """A DeviceBuffer holding a key whose trimmed layout the context has recorded (moai_key_register and the entry points that
    record): the record is dropped (moai_key_forget) before the block goes back to the allocator."""

    def __init__(self, ctx, n_words):
        super().__init__(n_words)
        self._ctx = ctx

    def free(self):
        if self.ptr and getattr(self._ctx, "h", None):
            lib().moai_key_forget(self._ctx.h, self.ptr)
        super().free()


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    return int(x)  # raw device pointer (e.g. torch.Tensor.data_ptr())


class Context:
    """moai_ctx: per-prime NTT tables and constants on the device, shared by all levels."""

    def __init__(self, coeff_count_power, primes, device=0):
        self.logn = int(coeff_count_power)
        self.n = 1 << self.logn
        self.primes = [int(p) for p in primes]
        self.k = len(self.primes)
        arr = (C.c_uint64 * self.k)(*self.primes)
        h = vp()
        _check(lib().moai_ctx_create(self.logn, arr, self.k, device, C.byref(h)))
        self.h = h.value

    def close(self):
        if getattr(self, "h", None):
            lib().moai_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, nbytes, stream=None):
        if stream is None:
            _check(lib().moai_ctx_reserve(self.h, int(nbytes)))
        else:
            _check(lib().moai_ctx_reserve_stream(self.h, stream, int(nbytes)))

    def root(self, i):
        return int(lib().moai_ctx_root(self.h, i))

    @staticmethod
    def _pidx(prime_index):
        if prime_index is None:
            return None
        return (C.c_uint32 * len(prime_index))(*[int(x) for x in prime_index])

    # --- raw-pointer API (device buffers) -----------------------------------------------------------
    def ntt_forward(self, data, n_poly, L, prime_index=None, stream=None):
        _check(lib().moai_ntt_forward(self.h, _ptr(data), n_poly, L, self._pidx(prime_index), stream))

    def ntt_inverse(self, data, n_poly, L, prime_index=None, stream=None):
        _check(lib().moai_ntt_inverse(self.h, _ptr(data), n_poly, L, self._pidx(prime_index), stream))

    def add(self, a, b, out, n_poly, L, stream=None):
        _check(lib().moai_add(self.h, _ptr(a), _ptr(b), _ptr(out), n_poly, L, stream))

    def sub(self, a, b, out, n_poly, L, stream=None):
        _check(lib().moai_sub(self.h, _ptr(a), _ptr(b), _ptr(out), n_poly, L, stream))

    def negate(self, a, out, n_poly, L, stream=None):
        _check(lib().moai_negate(self.h, _ptr(a), _ptr(out), n_poly, L, stream))

    def dyadic_mul(self, a, b, out, n_poly, n_poly_b, L, stream=None):
        _check(lib().moai_dyadic_mul(self.h, _ptr(a), _ptr(b), _ptr(out), n_poly, n_poly_b, L, stream))

    def mul_scalar_rows(self, a, scalars, out, n_poly, L, stream=None):
        s = (C.c_uint64 * L)(*[int(x) for x in scalars])
        _check(lib().moai_mul_scalar_rows(self.h, _ptr(a), s, _ptr(out), n_poly, L, stream))

    def add_scalar_rows(self, a, scalars, out, n_poly, L, stream=None):
        s = (C.c_uint64 * L)(*[int(x) for x in scalars])
        _check(lib().moai_add_scalar_rows(self.h, _ptr(a), s, _ptr(out), n_poly, L, stream))

    def mul_i_add(self, a, b, out, n_poly, L, sign=1, stream=None):
        """out = a + sign * X^(N/2) * b on NTT-form rows (a may be None: the plain monomial product)"""
        _check(lib().moai_mul_i_add(self.h, _ptr(a), _ptr(b), _ptr(out), n_poly, L, int(sign), stream))

    def real_split(self, r, rbar, out_re, out_im, n_poly, L, stream=None):
        """out_re = r + rbar, out_im = -X^(N/2) * (r - rbar)"""
        _check(lib().moai_real_split(self.h, _ptr(r), _ptr(rbar), _ptr(out_re), _ptr(out_im), n_poly, L, stream))

    def ct_multiply(self, x, y, out, L, batch, stream=None):
        _check(lib().moai_ct_multiply(self.h, _ptr(x), _ptr(y), _ptr(out), L, batch, stream))

    def ct_multiply_general(self, x, size_x, y, size_y, out, L, batch, stream=None):
        _check(lib().moai_ct_multiply_general(self.h, _ptr(x), size_x, _ptr(y), size_y, _ptr(out), L, batch, stream))

    def ct_square(self, x, out, L, batch, stream=None):
        _check(lib().moai_ct_square(self.h, _ptr(x), _ptr(out), L, batch, stream))

    def ct_dot(self, x, y, out, count, L, stream=None):
        _check(lib().moai_ct_dot(self.h, _ptr(x), _ptr(y), _ptr(out), count, L, stream))

    def ct_pt_dot(self, x, p, out, x_index, p_index, n_poly, L, stream=None):
        xi = (C.c_uint32 * len(x_index))(*[int(v) for v in x_index])
        pi = (C.c_uint32 * len(p_index))(*[int(v) for v in p_index])
        _check(lib().moai_ct_pt_dot(self.h, _ptr(x), _ptr(p), _ptr(out), xi, pi, len(x_index), n_poly, L, stream))

    def ct_pt_dot2(self, x, p, out, out2, x_index, p_index, p_index2, n_poly, L, stream=None):
        xi = (C.c_uint32 * len(x_index))(*[int(v) for v in x_index])
        pi = (C.c_uint32 * len(p_index))(*[int(v) for v in p_index])
        pi2 = (C.c_uint32 * max(1, len(p_index2)))(*[int(v) for v in p_index2])
        _check(lib().moai_ct_pt_dot2(self.h, _ptr(x), _ptr(p), _ptr(out), _ptr(out2), xi, pi, pi2, len(x_index), len(p_index2), n_poly, L,
                                     stream))

    def ct_pt_dot_rows(self, x, p, p2, out, out2, rows, n_poly, L, stream=None):
        _check(lib().moai_ct_pt_dot_rows(self.h, _ptr(x), _ptr(p), _ptr(p2) if p2 is not None else None, _ptr(out),
                                         _ptr(out2) if out2 is not None else None, rows, n_poly, L, stream))

    def ct_pt_matmul(self, x, w, out, rows, cols, size, L, stream=None):
        _check(lib().moai_ct_pt_matmul(self.h, _ptr(x), _ptr(w), _ptr(out), rows, cols, size, L, stream))

    def rescale(self, src, out, size, L, batch, stream=None):
        _check(lib().moai_rescale(self.h, _ptr(src), _ptr(out), size, L, batch, stream))

    def mul_scalar_rescale(self, src, scalars, out, size, L, batch, stream=None):
        s = (C.c_uint64 * L)(*[int(x) for x in scalars])
        _check(lib().moai_mul_scalar_rescale(self.h, _ptr(src), s, _ptr(out), size, L, batch, stream))

    def rescale_add(self, src, addend, out, size, L, batch, stream=None):
        _check(lib().moai_rescale_add(self.h, _ptr(src), _ptr(addend), _ptr(out), size, L, batch, stream))

    def mul_scalar_rescale_add(self, src, scalars, addend, out, size, L, batch, stream=None):
        s = (C.c_uint64 * L)(*[int(x) for x in scalars])
        _check(lib().moai_mul_scalar_rescale_add(self.h, _ptr(src), s, _ptr(addend), _ptr(out), size, L, batch, stream))

    def mod_drop(self, src, out, size, L, drop, batch, stream=None):
        _check(lib().moai_mod_drop(self.h, _ptr(src), _ptr(out), size, L, drop, batch, stream))

    def galois_permute(self, src, out, n_poly, L, elt, stream=None):
        _check(lib().moai_galois_permute(self.h, _ptr(src), _ptr(out), n_poly, L, int(elt), stream))

    def galois_elt_from_step(self, step):
        e = lib().moai_galois_elt_from_step(self.h, int(step))
        if e == 0:
            raise MoaiError(-1, lib().moai_last_error().decode())
        return int(e)

    def switch_key(self, ct, target, key, L, batch, stream=None):
        _check(lib().moai_switch_key(self.h, _ptr(ct), _ptr(target), _ptr(key), L, batch, stream))

    def relinearize(self, ct3, key, out, L, batch, stream=None):
        _check(lib().moai_relinearize(self.h, _ptr(ct3), _ptr(key), _ptr(out), L, batch, stream))

    def apply_galois_acc(self, src, acc, L, elt, key, batch, stream=None):
        _check(lib().moai_apply_galois_acc(self.h, _ptr(src), _ptr(acc), L, int(elt), _ptr(key), batch, stream))

    def apply_galois(self, ct, L, elt, key, batch, stream=None):
        _check(lib().moai_apply_galois(self.h, _ptr(ct), L, int(elt), _ptr(key), batch, stream))

    # hybrid key switching (include/moai_hip.h, "hybrid key switching"): alpha special primes, digits of alpha primes
    def hybrid_digits(self, alpha, L):
        """beta(L) = ceil(L / alpha) for a level of L <= k - alpha data primes"""
        d = lib().moai_hybrid_digits(self.h, alpha, L)
        if d == 0:
            _check(MOAI_EINVAL)
        return int(d)

    # include/moai_hip.h, "hybrid rounding mode": HYBRID_ROUND_FAST (the default) or HYBRID_ROUND_EXACT, per context
    def hybrid_set_rounding(self, mode):
        _check(lib().moai_hybrid_set_rounding(self.h, int(mode)))

    def hybrid_rounding(self):
        mode = C.c_int(-1)
        _check(lib().moai_hybrid_rounding(self.h, C.byref(mode)))
        return mode.value

    def switch_key_hybrid(self, ct, target, key, L, alpha, batch, stream=None):
        _check(lib().moai_switch_key_hybrid(self.h, _ptr(ct), _ptr(target), _ptr(key), L, alpha, batch, stream))

    def relinearize_hybrid(self, ct3, key, out, L, alpha, batch, stream=None):
        _check(lib().moai_relinearize_hybrid(self.h, _ptr(ct3), _ptr(key), _ptr(out), L, alpha, batch, stream))

    def relinearize_rescale_hybrid(self, ct3, key, out, L, alpha, batch, stream=None):
        """out [batch][2][L-1][N] = relinearize_hybrid + rescale of ct3 [batch][3][L][N] with ONE mod-down by P q_{L-1} (its own
        documented rounding, not the composition's bits)"""
        _check(lib().moai_relinearize_rescale_hybrid(self.h, _ptr(ct3), _ptr(key), _ptr(out), L, alpha, batch, stream))

    def multiply_relin_rescale_hybrid(self, x, y, key, out, L, alpha, batch, stream=None):
        """ct_multiply (ct_square where y is x) followed by relinearize_rescale_hybrid; the product stays in scratch"""
        _check(lib().moai_multiply_relin_rescale_hybrid(self.h, _ptr(x), _ptr(y), _ptr(key), _ptr(out), L, alpha, batch, stream))

    def apply_galois_hybrid(self, ct, L, alpha, elt, key, batch, stream=None):
        _check(lib().moai_apply_galois_hybrid(self.h, _ptr(ct), L, alpha, int(elt), _ptr(key), batch, stream))

    # hybrid key switches on a list of ciphertexts (include/moai_hip.h, "hybrid key switches on a list of ciphertexts")
    def apply_galois_hybrid_to(self, src, dst, L, alpha, elt, key, batch, stream=None):
        """dst = apply_galois_hybrid(copy of src); dst may be src"""
        _check(lib().moai_apply_galois_hybrid_to(self.h, _ptr(src), _ptr(dst), L, alpha, int(elt), _ptr(key), batch, stream))

    def apply_galois_hybrid_acc(self, src, acc, L, alpha, elt, key, batch, stream=None):
        """acc += apply_galois_hybrid(copy of src): the addition rides on the switch's last kernel"""
        _check(lib().moai_apply_galois_hybrid_acc(self.h, _ptr(src), _ptr(acc), L, alpha, int(elt), _ptr(key), batch, stream))

    def apply_galois_hybrid_ptrs(self, ins, outs, L, alpha, elts, keys, sums=None, stream=None):
        """outs[i] = [sums[i] +] apply_galois_hybrid(copy of ins[i], elts[i], keys[i]) for single ciphertexts [2][L][N] in separate
        buffers, in one chain of launches; sums: None, or a list whose entries may be None"""
        n = len(ins)
        ai = (vp * n)(*[_ptr(x) for x in ins])
        ao = (vp * n)(*[_ptr(x) for x in outs])
        e = (C.c_uint32 * n)(*[int(x) for x in elts])
        ak = (vp * n)(*[_ptr(x) for x in keys])
        asum = None if sums is None else (vp * n)(*[_ptr(x) for x in sums])
        _check(lib().moai_apply_galois_hybrid_ptrs(self.h, ai, ao, L, alpha, e, ak, asum, n, stream))

    def relinearize_hybrid_ptrs(self, ct3s, outs, key, L, alpha, stream=None):
        """outs[i] [2][L][N] = relinearize_hybrid(ct3s[i] [3][L][N]) with one key, in one chain of launches"""
        n = len(ct3s)
        ai = (vp * n)(*[_ptr(x) for x in ct3s])
        ao = (vp * n)(*[_ptr(x) for x in outs])
        _check(lib().moai_relinearize_hybrid_ptrs(self.h, ai, ao, _ptr(key), L, alpha, n, stream))

    def relinearize_rescale_hybrid_ptrs(self, ct3s, outs, key, L, alpha, stream=None):
        """outs[i] [2][L-1][N] = relinearize_rescale_hybrid(ct3s[i] [3][L][N]) with one key, in one chain of launches"""
        n = len(ct3s)
        ai = (vp * n)(*[_ptr(x) for x in ct3s])
        ao = (vp * n)(*[_ptr(x) for x in outs])
        _check(lib().moai_relinearize_rescale_hybrid_ptrs(self.h, ai, ao, _ptr(key), L, alpha, n, stream))

    def hybrid_hoist_correction(self, key, elt, L, alpha, stream=None):
        """the per-(key, element, level) constant of the hoisted hybrid rotations: DeviceBuffer [2][L+alpha][N]"""
        out = DeviceBuffer(2 * (L + alpha) * self.n)
        _check(lib().moai_hybrid_hoist_correction(self.h, _ptr(key), int(elt), L, alpha, _ptr(out), stream))
        return out

    def apply_galois_hybrid_hoisted(self, src, dst, L, alpha, elts, keys, corrections, batch, stream=None):
        """dst[r] = apply_galois_hybrid(copy of src, elts[r], keys[r]) for every r with one digit decomposition (dst: one buffer
        [R][batch][2][L][N] or a list of R buffers); returns True when the library had to fall back to separate calls (a zero
        coefficient in INTT(c1))"""
        R = len(elts)
        if isinstance(dst, (list, tuple)):
            op = (vp * R)(*[_ptr(d) for d in dst])
        else:
            words = batch * 2 * L * self.n * 8
            op = (vp * R)(*[_ptr(dst) + r * words for r in range(R)])
        e = (C.c_uint32 * R)(*[int(x) for x in elts])
        kp = (vp * R)(*[_ptr(k) for k in keys])
        cp = (vp * R)(*[_ptr(k) for k in corrections])
        fb = C.c_int(0)
        _check(lib().moai_apply_galois_hybrid_hoisted(self.h, _ptr(src), op, L, alpha, e, kp, cp, R, batch, C.byref(fb), stream))
        return bool(fb.value)

    def hybrid_rotate_pt_dot(self, src, dsts, L, alpha, elts, keys, corrections, plains, batch, stream=None):
        """dsts[g] = sum_r plains[g][r] (*) rotation elts[r] of src, summed in the extended basis with one mod-down per output
        (dsts: one buffer [n_out][batch][2][L][N] or a list of n_out buffers; plains: n_out lists of R buffers [L+alpha][N] or None
        for an absent term; keys[r] and corrections[r] may be None where elts[r] is 1); returns True when a chunk took the
        unhoisted route (a zero coefficient in INTT(c1))"""
        R, n_out = len(elts), len(plains)
        if isinstance(dsts, (list, tuple)):
            op = (vp * n_out)(*[_ptr(d) for d in dsts])
        else:
            words = batch * 2 * L * self.n * 8
            op = (vp * n_out)(*[_ptr(dsts) + g * words for g in range(n_out)])
        e = (C.c_uint32 * R)(*[int(x) for x in elts])
        kp = (vp * R)(*[_ptr(k) for k in keys])
        cp = (vp * R)(*[_ptr(k) for k in corrections])
        pp = (vp * (n_out * R))(*[_ptr(p) for row in plains for p in row])
        fb = C.c_int(0)
        _check(lib().moai_hybrid_rotate_pt_dot(self.h, _ptr(src), op, n_out, L, alpha, e, kp, cp, R, pp, batch, C.byref(fb), stream))
        return bool(fb.value)

    def hybrid_bsgs_dot(self, src, dst, L, alpha, baby_elts, baby_keys, baby_corrections, giant_elts, giant_keys, plains, batch,
                        stream=None):
        """dst = sum_g rotation giant_elts[g] of (sum_r plains[g][r] (*) rotation baby_elts[r] of src), everything summed in the
        extended basis with one final mod-down (dst [batch][2][L][N]; plains: n_giant lists of R buffers [L+alpha][N] or None for an
        absent term; keys and corrections may be None where the element is 1); returns True when a chunk's inner stage took the
        unhoisted route (a zero coefficient in INTT(c1))"""
        R, ng = len(baby_elts), len(giant_elts)
        e = (C.c_uint32 * R)(*[int(x) for x in baby_elts])
        kp = (vp * R)(*[_ptr(k) for k in baby_keys])
        cp = (vp * R)(*[_ptr(k) for k in baby_corrections])
        ge = (C.c_uint32 * ng)(*[int(x) for x in giant_elts])
        gk = (vp * ng)(*[_ptr(k) for k in giant_keys])
        pp = (vp * (ng * R))(*[_ptr(p) for row in plains for p in row])
        fb = C.c_int(0)
        _check(lib().moai_hybrid_bsgs_dot(self.h, _ptr(src), _ptr(dst), L, alpha, e, kp, cp, R, ge, gk, ng, pp, batch, C.byref(fb), stream))
        return bool(fb.value)

    def apply_galois_to(self, src, dst, L, elt, key, batch, stream=None):
        _check(lib().moai_apply_galois_to(self.h, _ptr(src), _ptr(dst), L, int(elt), _ptr(key), batch, stream))

    def scalar_dot(self, xs, scalars, base, out, size, L, stream=None):
        """out = base + sum_t xs[t] (*) scalars[t] (scalars: numpy uint64 [terms][L], reduced)"""
        T = len(xs)
        arr = (vp * T)(*[_ptr(x) for x in xs])
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        _check(lib().moai_scalar_dot(self.h, arr, sc.ctypes.data_as(u64p), T, _ptr(base), _ptr(out), size, L, stream))

    def vector_dot(self, xs, plains, base, out, size, L, stream=None):
        """out = base + sum_t xs[t] (*) plains[t] (plains: one device buffer [terms][L][N])"""
        T = len(xs)
        arr = (vp * T)(*[_ptr(x) for x in xs])
        _check(lib().moai_vector_dot(self.h, arr, _ptr(plains), T, _ptr(base), _ptr(out), size, L, stream))

    def ct_dot_ptrs(self, xs, ys, base, out, L, stream=None):
        """out[3][L][N] = base + sum_t multiply(xs[t], ys[t]) for size-2 ciphertexts in separate buffers"""
        T = len(xs)
        ax = (vp * T)(*[_ptr(x) for x in xs])
        ay = (vp * T)(*[_ptr(y) for y in ys])
        _check(lib().moai_ct_dot_ptrs(self.h, ax, ay, T, _ptr(base), _ptr(out), L, stream))

    def apply_galois_ptrs(self, ins, outs, L, elts, keys, sums=None, stream=None):
        """outs[i] = [sums[i] +] apply_galois(ins[i], elts[i], keys[i]) for single ciphertexts [2][L][N] in separate buffers, in
        one chain of launches; sums: None, or a list whose entries may be None"""
        n = len(ins)
        ai = (vp * n)(*[_ptr(x) for x in ins])
        ao = (vp * n)(*[_ptr(x) for x in outs])
        e = (C.c_uint32 * n)(*[int(x) for x in elts])
        ak = (vp * n)(*[_ptr(x) for x in keys])
        asum = None if sums is None else (vp * n)(*[_ptr(x) for x in sums])
        _check(lib().moai_apply_galois_ptrs(self.h, ai, ao, L, e, ak, asum, n, stream))

    def relinearize_ptrs(self, ct3s, outs, key, L, stream=None):
        """outs[i] [2][L][N] = relinearize(ct3s[i] [3][L][N]) with one key, in one chain of launches"""
        n = len(ct3s)
        ai = (vp * n)(*[_ptr(x) for x in ct3s])
        ao = (vp * n)(*[_ptr(x) for x in outs])
        _check(lib().moai_relinearize_ptrs(self.h, ai, ao, _ptr(key), L, n, stream))

    def gather_blocks(self, blocks, packed, words, stream=None):
        """packed[i] = blocks[i] (`words` 64-bit words each) in one launch"""
        n = len(blocks)
        arr = (vp * n)(*[_ptr(b) for b in blocks])
        _check(lib().moai_gather_blocks(self.h, arr, _ptr(packed), n, words, stream))

    def scatter_blocks(self, packed, blocks, words, stream=None):
        """blocks[i] = packed[i] in one launch"""
        n = len(blocks)
        arr = (vp * n)(*[_ptr(b) for b in blocks])
        _check(lib().moai_scatter_blocks(self.h, _ptr(packed), arr, n, words, stream))

    def key_trim(self, full_key, levels, stream=None):
        """the part of a key a switch at <= `levels` data primes reads, as a DeviceBuffer [levels][2][levels+1][N] whose layout the
        context knows (moai_key_trim); pass it wherever a key is expected"""
        out = DeviceBuffer(lib().moai_key_words(self.h, levels))
        _check(lib().moai_key_trim(self.h, _ptr(full_key), levels, out.ptr, stream))
        _check(lib().moai_stream_sync(stream))
        return out

    def key_forget(self, key):
        _check(lib().moai_key_forget(self.h, _ptr(key)))

    def key_register(self, key, levels):
        """record the trimmed layout [levels][2][levels+1][N] for a block filled elsewhere (moai_key_register); key_forget before
        the block is freed or reused"""
        _check(lib().moai_key_register(self.h, _ptr(key), levels))

    def _key_buffer(self, levels):
        words = lib().moai_key_words(self.h, levels) if 1 <= levels <= self.k - 1 else 0
        return KeyBuffer(self, max(words, 2))  # out-of-range levels: the library reports them

    def kswitch_keygen_limited(self, key, seq, sk_ntt, new_key_ntt, levels, stream=None):
        """The switching key for new_key_ntt [k][N] limited to `levels` data primes: a KeyBuffer [levels][2][levels+1][N] whose
        layout the context knows, word for word key_trim(kswitch_keygen(key, seq, ...), levels)"""
        out = self._key_buffer(levels)
        _check(lib().moai_kswitch_keygen_limited(self.h, self._key(key), int(seq), _ptr(sk_ntt), _ptr(new_key_ntt), levels, out.ptr,
                                                 stream))
        return out

    def kswitch_keygen_limited_seeded(self, noise_key, seed, seq, sk_ntt, new_key_ntt, levels, stream=None):
        """c0 [levels][levels+1][N] of the limited switching key (nothing is recorded)"""
        out = DeviceBuffer(max(levels * (levels + 1), 1) * self.n)
        _check(lib().moai_kswitch_keygen_limited_seeded(self.h, self._key(noise_key), self._key(seed), int(seq), _ptr(sk_ntt),
                                                        _ptr(new_key_ntt), levels, out.ptr, stream))
        return out

    def expand_seeded_limited(self, seed, seq, c0, levels, stream=None):
        """c0 [levels][levels+1][N] -> a usable limited key, a KeyBuffer [levels][2][levels+1][N] whose layout the context knows"""
        out = self._key_buffer(levels)
        _check(lib().moai_expand_seeded_limited(self.h, self._key(seed), int(seq), _ptr(c0), levels, out.ptr, stream))
        return out

    def hoist_correction(self, key, elt, L, stream=None):
        """the per-(key, level) constant of the hoisted rotations: DeviceBuffer [2][L+1][N]"""
        out = DeviceBuffer(2 * (L + 1) * self.n)
        _check(lib().moai_hoist_correction(self.h, _ptr(key), int(elt), L, _ptr(out), stream))
        return out

    def apply_galois_hoisted(self, src, dst, L, elts, keys, corrections, batch, stream=None):
        """dst[r] = apply_galois(src, elts[r], keys[r]) for every r with one digit decomposition (dst: one buffer
        [R][batch][2][L][N] or a list of R buffers); returns True when the library had to fall back to separate calls (a
        zero coefficient in INTT(c1))"""
        R = len(elts)
        if isinstance(dst, (list, tuple)):
            op = (vp * R)(*[_ptr(d) for d in dst])
        else:
            words = batch * 2 * L * self.n * 8
            op = (vp * R)(*[_ptr(dst) + r * words for r in range(R)])
        e = (C.c_uint32 * R)(*[int(x) for x in elts])
        kp = (vp * R)(*[_ptr(k) for k in keys])
        cp = (vp * R)(*[_ptr(k) for k in corrections])
        fb = C.c_int(0)
        _check(lib().moai_apply_galois_hoisted(self.h, _ptr(src), op, L, e, kp, cp, R, batch, C.byref(fb), stream))
        return bool(fb.value)

    def modraise(self, src, out, L_out, batch, stream=None):
        _check(lib().moai_modraise(self.h, _ptr(src), _ptr(out), L_out, batch, stream))

    def ckks_encode(self, values, L, scale, prime_index=None, stream=None):
        """CKKSEncoder::encode for a batch of vectors: values [n_batch][count] float64 or complex128 (host).
        Returns (DeviceBuffer [n_batch][L][N] in NTT form, max |coefficient| per vector); raises like
        the reference when a vector does not fit the level's modulus (SEAL/ckks.h:527-538)."""
        v = np.asarray(values)
        is_complex = np.iscomplexobj(v)
        v = np.ascontiguousarray(v, dtype=np.complex128 if is_complex else np.float64)
        if v.ndim == 1:
            v = v[None, :]
        n_batch, count = v.shape
        words = v.size * (2 if is_complex else 1)
        dv = DeviceBuffer(max(words, 1) + n_batch)
        _check(lib().moai_memcpy_h2d(dv.ptr, v.ctypes.data, words * 8, stream))
        out = DeviceBuffer(n_batch * L * self.n)
        mx_ptr = dv.ptr + max(words, 1) * 8
        _check(lib().moai_ckks_encode(self.h, dv.ptr, 1 if is_complex else 0, count, n_batch, out.ptr, L,
                                      self._pidx(prime_index), float(scale), mx_ptr, stream))
        mx = np.empty(n_batch, dtype=np.float64)
        _check(lib().moai_stream_sync(stream))
        _check(lib().moai_memcpy_d2h(mx.ctypes.data, mx_ptr, n_batch * 8, stream))
        _check(lib().moai_stream_sync(stream))
        total = self.total_coeff_modulus_bit_count(L, prime_index)
        bits = np.ceil(np.log2(np.maximum(mx, 1.0))).astype(int) + 1
        if np.any(bits >= total) or not np.all(np.isfinite(mx)):
            raise MoaiError(MOAI_EINVAL, "encoded values are too large")
        return out, mx

    def ckks_encode_masked(self, constants, mask, L, scale, prime_index=None, stream=None):
        """moai_ckks_encode_masked: vector b = constants[b] on the slots where mask == 1, 0 elsewhere."""
        cst = np.ascontiguousarray(constants, dtype=np.float64)
        msk = np.ascontiguousarray(mask, dtype=np.int32)
        n_batch = cst.size
        dc = DeviceBuffer(2 * n_batch + 1)
        dm = DeviceBuffer((msk.size + 1) // 2 + 1)
        _check(lib().moai_memcpy_h2d(dc.ptr, cst.ctypes.data, n_batch * 8, stream))
        _check(lib().moai_memcpy_h2d(dm.ptr, msk.ctypes.data, msk.size * 4, stream))
        out = DeviceBuffer(n_batch * L * self.n)
        mx_ptr = dc.ptr + n_batch * 8
        _check(lib().moai_ckks_encode_masked(self.h, dc.ptr, dm.ptr, msk.size, n_batch, out.ptr, L,
                                             self._pidx(prime_index), float(scale), mx_ptr, stream))
        mx = np.empty(n_batch, dtype=np.float64)
        _check(lib().moai_stream_sync(stream))
        _check(lib().moai_memcpy_d2h(mx.ctypes.data, mx_ptr, n_batch * 8, stream))
        _check(lib().moai_stream_sync(stream))
        return out, mx

    def decrypt(self, ct, size, sk_ntt, L, n_batch=1, prime_index=None, stream=None):
        """Decryptor::decrypt for a batch: ct [n_batch][size][L][N] and sk_ntt [L][N] (device buffers or pointers).
        Returns a DeviceBuffer [n_batch][L][N] holding c_0 + c_1 s + ... in NTT form."""
        out = DeviceBuffer(max(n_batch, 1) * L * self.n)
        _check(lib().moai_decrypt(self.h, _ptr(ct), size, _ptr(sk_ntt), out.ptr, n_batch, L,
                                  self._pidx(prime_index), stream))
        return out

    def ckks_decode(self, plain, L, scales, n_batch=1, prime_index=None, is_complex=False, stream=None):
        """CKKSEncoder::decode of n_batch NTT-form plaintexts plain [n_batch][L][N] (device buffer or pointer) at
        scales (one float, or one per plaintext).  Returns numpy [n_batch][N/2], float64 or complex128."""
        sc = np.broadcast_to(np.asarray(scales, dtype=np.float64), (n_batch,))
        sc = np.ascontiguousarray(sc)
        slots = self.n // 2
        words = max(n_batch, 1) * slots * (2 if is_complex else 1)
        out = DeviceBuffer(words)
        _check(lib().moai_ckks_decode(self.h, _ptr(plain), n_batch, L, self._pidx(prime_index),
                                      sc.ctypes.data_as(C.POINTER(C.c_double)), 1 if is_complex else 0, out.ptr, stream))
        host = np.empty(words, dtype=np.float64)
        _check(lib().moai_memcpy_d2h(host.ctypes.data, out.ptr, words * 8, stream))
        _check(lib().moai_stream_sync(stream))
        host = host[: n_batch * slots * (2 if is_complex else 1)]
        if is_complex:
            return host.view(np.complex128).reshape(n_batch, slots)
        return host.reshape(n_batch, slots)

    def ckks_decode_sparse(self, plain, L, scales, sparse_slots, n_batch=1, prime_index=None, is_complex=False, stream=None):
        """CKKSEncoder::decode with sparse_slots set: the projection onto the sparse subring, then the first sparse_slots
        slots.  Returns numpy [n_batch][sparse_slots], float64 or complex128."""
        sc = np.broadcast_to(np.asarray(scales, dtype=np.float64), (n_batch,))
        sc = np.ascontiguousarray(sc)
        slots = int(sparse_slots)
        if slots < 1:
            raise ValueError("sparse_slots must be a power of two in [1, N/2]")
        words = max(n_batch, 1) * slots * (2 if is_complex else 1)
        out = DeviceBuffer(words)
        _check(lib().moai_ckks_decode_sparse(self.h, _ptr(plain), n_batch, L, self._pidx(prime_index),
                                             sc.ctypes.data_as(C.POINTER(C.c_double)), slots, 1 if is_complex else 0,
                                             out.ptr, stream))
        host = np.empty(words, dtype=np.float64)
        _check(lib().moai_memcpy_d2h(host.ctypes.data, out.ptr, words * 8, stream))
        _check(lib().moai_stream_sync(stream))
        host = host[: n_batch * slots * (2 if is_complex else 1)]
        if is_complex:
            return host.view(np.complex128).reshape(n_batch, slots)
        return host.reshape(n_batch, slots)

    # --- client randomness and encryption (include/moai_hip.h, "client randomness and encryption") -----------------
    @staticmethod
    def _key(key):
        if key is None:
            return None
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("a ChaCha20 key has 32 bytes")
        return key

    def _sample(self, fn, key, nonce, n_poly, L, prime_index, stream):
        out = DeviceBuffer(max(n_poly, 1) * L * self.n)
        _check(fn(self.h, self._key(key), int(nonce), out.ptr, n_poly, L, self._pidx(prime_index), stream))
        return out

    def sample_uniform(self, key, nonce, n_poly, L, prime_index=None, stream=None):
        """[n_poly][L][N] uniform residues; polynomial p from the stream (key, nonce + p)."""
        return self._sample(lib().moai_sample_uniform, key, nonce, n_poly, L, prime_index, stream)

    def sample_ternary(self, key, nonce, n_poly, L, prime_index=None, stream=None):
        """[n_poly][L][N] residues of one ternary polynomial each."""
        return self._sample(lib().moai_sample_ternary, key, nonce, n_poly, L, prime_index, stream)

    def sample_cbd(self, key, nonce, n_poly, L, prime_index=None, stream=None):
        """[n_poly][L][N] residues of one centred-binomial noise polynomial each."""
        return self._sample(lib().moai_sample_cbd, key, nonce, n_poly, L, prime_index, stream)

    def encrypt_symmetric(self, key, seq, sk_ntt, L, n_batch=1, plain=None, prime_index=None, stream=None):
        """Encryptor::encrypt_symmetric of n_batch plaintexts [n_batch][L][N] (None: encryptions of zero) under sk_ntt [L][N].
        Returns a DeviceBuffer [n_batch][2][L][N]."""
        out = DeviceBuffer(max(n_batch, 1) * 2 * L * self.n)
        _check(lib().moai_encrypt_symmetric(self.h, self._key(key), int(seq), _ptr(sk_ntt), _ptr(plain), out.ptr, n_batch, L,
                                            self._pidx(prime_index), stream))
        return out

    def encrypt_asymmetric(self, key, seq, pk, L, n_batch=1, plain=None, stream=None):
        """Encryptor::encrypt with the key-level public key pk [2][k][N] at the level of L primes.
        Returns a DeviceBuffer [n_batch][2][L][N]."""
        out = DeviceBuffer(max(n_batch, 1) * 2 * L * self.n)
        _check(lib().moai_encrypt_asymmetric(self.h, self._key(key), int(seq), _ptr(pk), _ptr(plain), out.ptr, n_batch, L, stream))
        return out

    def kswitch_keygen(self, key, seq, sk_ntt, new_key_ntt, stream=None):
        """The k-1 digits of the switching key for new_key_ntt [k][N]: a DeviceBuffer [k-1][2][k][N]."""
        out = DeviceBuffer(max(self.k - 1, 1) * 2 * self.k * self.n)
        _check(lib().moai_kswitch_keygen(self.h, self._key(key), int(seq), _ptr(sk_ntt), _ptr(new_key_ntt), out.ptr, stream))
        return out

    def hybrid_keygen(self, key, seq, sk_ntt, new_key_ntt, alpha, stream=None):
        """The beta(k - alpha) digits of the hybrid switching key for new_key_ntt [k][N]: a DeviceBuffer [beta][2][k][N]."""
        digits = self.hybrid_digits(alpha, self.k - alpha)
        out = DeviceBuffer(digits * 2 * self.k * self.n)
        _check(lib().moai_hybrid_keygen(self.h, self._key(key), int(seq), _ptr(sk_ntt), _ptr(new_key_ntt), alpha, out.ptr, stream))
        return out

    # --- wire form (include/moai_hip.h, "wire form: seeded objects and bit-packed rows") ---------------------------
    def packed_words(self, L, prime_index=None):
        """64-bit words of one packed polynomial of L rows"""
        w = lib().moai_packed_words(self.h, L, self._pidx(prime_index))
        if w == 0:
            _check(MOAI_EINVAL)
        return w

    def pack_rows(self, data, n_poly, L, prime_index=None, stream=None):
        """[n_poly][L][N] residues -> a DeviceBuffer of n_poly * packed_words(L) words, every row at its prime's bit length"""
        out = DeviceBuffer(max(n_poly, 1) * self.packed_words(L, prime_index))
        _check(lib().moai_pack_rows(self.h, _ptr(data), out.ptr, n_poly, L, self._pidx(prime_index), stream))
        return out

    def unpack_rows(self, packed, n_poly, L, prime_index=None, check=True, stream=None):
        """the inverse of pack_rows: (DeviceBuffer [n_poly][L][N], invalid); invalid is True when a field held a value >= its
        row's prime (None with check=False, which hands the library no flag)"""
        out = DeviceBuffer(max(n_poly, 1) * L * self.n)
        flag = DeviceBuffer(1) if check else None
        if check:
            _check(lib().moai_memset_zero(flag.ptr, 8, stream))
        _check(lib().moai_unpack_rows(self.h, _ptr(packed), out.ptr, n_poly, L, self._pidx(prime_index), _ptr(flag), stream))
        return out, (bool(flag.to_numpy(stream=stream)[0]) if check else None)

    def encrypt_symmetric_seeded(self, noise_key, seed, seq, sk_ntt, L, n_batch=1, plain=None, prime_index=None, stream=None):
        """c0 [n_batch][L][N] of encrypt_symmetric with a drawn from the public `seed` and the noise from `noise_key`"""
        out = DeviceBuffer(max(n_batch, 1) * L * self.n)
        _check(lib().moai_encrypt_symmetric_seeded(self.h, self._key(noise_key), self._key(seed), int(seq), _ptr(sk_ntt), _ptr(plain),
                                                   out.ptr, n_batch, L, self._pidx(prime_index), stream))
        return out

    def kswitch_keygen_seeded(self, noise_key, seed, seq, sk_ntt, new_key_ntt, stream=None):
        """c0 [k-1][k][N] of the k-1 digits of the switching key for new_key_ntt"""
        out = DeviceBuffer(max(self.k - 1, 1) * self.k * self.n)
        _check(lib().moai_kswitch_keygen_seeded(self.h, self._key(noise_key), self._key(seed), int(seq), _ptr(sk_ntt),
                                                _ptr(new_key_ntt), out.ptr, stream))
        return out

    def expand_seeded(self, seed, seq, c0, count, L, prime_index=None, stream=None):
        """[count][L][N] -> [count][2][L][N] with c1 drawn from (seed, sequence seq + b)"""
        out = DeviceBuffer(max(count, 1) * 2 * L * self.n)
        _check(lib().moai_expand_seeded(self.h, self._key(seed), int(seq), _ptr(c0), out.ptr, count, L, self._pidx(prime_index), stream))
        return out

    # --- SEAL's own format (include/moai_hip.h, "SEAL's own format: the generator of seeded objects") --------------
    def seal_prng_bytes(self, seed, first_block, n_blocks, stream=None):
        """buffers first_block .. first_block + n_blocks - 1 (4096 bytes each) of SEAL's Blake2xbPRNG(seed), as bytes"""
        seed = bytes(seed)
        if len(seed) != 64:
            raise ValueError("a SEAL generator seed has 64 bytes")
        out = DeviceBuffer(max(n_blocks, 1) * 512)
        _check(lib().moai_seal_prng_bytes(self.h, seed, int(first_block), int(n_blocks), out.ptr, stream))
        return out.to_numpy(stream=stream, words=n_blocks * 512).astype("<u8").tobytes()

    def seal_sample_uniform(self, seeds, L, out=None, stride_words=None, prime_index=None, count_rejected=True, stream=None):
        """sample_poly_uniform from a fresh Blake2xbPRNG per seed (64 bytes each): polynomial b lands at out + b * stride_words
        as [L][N] (a new DeviceBuffer [count][L][N] when out is None).  Returns (DeviceBuffer or None, rejected, overflow):
        the stream words rejected and whether a tail ran over its bound (None, None with count_rejected=False)."""
        seeds = [bytes(s) for s in seeds]
        if any(len(s) != 64 for s in seeds):
            raise ValueError("a SEAL generator seed has 64 bytes")
        stride_words = L * self.n if stride_words is None else stride_words
        made = DeviceBuffer(max(len(seeds), 1) * stride_words) if out is None else None
        flag = self._rejected_flag(count_rejected, stream)
        _check(lib().moai_seal_sample_uniform(self.h, b"".join(seeds), _ptr(made if out is None else out), stride_words, len(seeds), L,
                                              self._pidx(prime_index), _ptr(flag), stream))
        return (made,) + self._rejected_words(flag, stream)

    @staticmethod
    def _rejected_flag(count_rejected, stream):
        """a zeroed device uint32_t[2] for a `rejected` argument, or None"""
        flag = DeviceBuffer(1) if count_rejected else None
        if count_rejected:
            _check(lib().moai_memset_zero(flag.ptr, 8, stream))
        return flag

    @staticmethod
    def _rejected_words(flag, stream):
        """(rejected stream words, whether a tail ran over its bound), (None, None) without a flag"""
        if flag is None:
            return None, None
        word = int(flag.to_numpy(stream=stream)[0])
        return word & 0xFFFFFFFF, bool(word >> 32)

    @staticmethod
    def _seal_seeds(seeds, count):
        seeds = [bytes(s) for s in seeds]
        if len(seeds) != count or any(len(s) != 64 for s in seeds):
            raise ValueError("%d SEAL generator seeds of 64 bytes each are needed" % count)
        return b"".join(seeds)

    def encrypt_symmetric_seal_seeded(self, noise_key, seeds, seq, sk_ntt, L, plain=None, prime_index=None, count_rejected=True,
                                      stream=None):
        """c0 [len(seeds)][L][N] of encrypt_symmetric with a of ciphertext b = SEAL's sample_poly_uniform of seeds[b] (64 bytes
        each) and the noise from `noise_key`.  Returns (DeviceBuffer, rejected, overflow) as seal_sample_uniform does."""
        n_batch = len(seeds)
        out = DeviceBuffer(max(n_batch, 1) * L * self.n)
        flag = self._rejected_flag(count_rejected, stream)
        _check(lib().moai_encrypt_symmetric_seal_seeded(self.h, self._key(noise_key), self._seal_seeds(seeds, n_batch), int(seq),
                                                        _ptr(sk_ntt), _ptr(plain), out.ptr, n_batch, L, self._pidx(prime_index),
                                                        _ptr(flag), stream))
        return (out,) + self._rejected_words(flag, stream)

    def kswitch_keygen_seal_seeded(self, noise_key, seeds, seq, sk_ntt, new_key_ntt, count_rejected=True, stream=None):
        """c0 [k-1][k][N] of the k-1 digits of the switching key for new_key_ntt, a of digit J from the SEAL seed seeds[J].
        Returns (DeviceBuffer, rejected, overflow)."""
        out = DeviceBuffer(max(self.k - 1, 1) * self.k * self.n)
        flag = self._rejected_flag(count_rejected, stream)
        _check(lib().moai_kswitch_keygen_seal_seeded(self.h, self._key(noise_key), self._seal_seeds(seeds, self.k - 1), int(seq),
                                                     _ptr(sk_ntt), _ptr(new_key_ntt), out.ptr, _ptr(flag), stream))
        return (out,) + self._rejected_words(flag, stream)

    def check_residues(self, data, n_poly, L, prime_index=None, stream=None):
        """True when a residue of data [n_poly][L][N] is >= its row's prime"""
        flag = DeviceBuffer(1)
        _check(lib().moai_memset_zero(flag.ptr, 8, stream))
        _check(lib().moai_check_residues(self.h, _ptr(data), n_poly, L, self._pidx(prime_index), flag.ptr, stream))
        return bool(flag.to_numpy(stream=stream)[0])

    def total_coeff_modulus_bit_count(self, L, prime_index=None):
        r = lib().moai_total_coeff_modulus_bit_count(self.h, L, self._pidx(prime_index))
        if r == 0:
            _check(MOAI_EINVAL)
        return r

    def ckks_tables(self):
        idx = np.empty(self.n, dtype=np.uint32)
        roots = np.empty((self.n, 2), dtype=np.float64)
        _check(lib().moai_ckks_tables(self.h, idx.ctypes.data, roots.ctypes.data))
        return idx, roots

    def arith_mode(self, prime, op, L=0, rows=0):
        """the arithmetic mode (MODE_*) that operation `op` (MODE_OF_*) takes now for context prime `prime`: the key switch at L
        data primes and rows = batch ciphertexts, mod-down / rescale with rows = polynomials * kept primes, or the plain
        forward / inverse transform (moai_arith_mode; no launch)"""
        m = C.c_int(0)
        _check(lib().moai_arith_mode(self.h, int(prime), int(op), int(L), int(rows), C.byref(m)))
        return m.value

    def sync(self, stream=None):
        _check(lib().moai_stream_sync(stream))


def set_tuning(name, value):
    _check(lib().moai_set_tuning(name.encode(), int(value)))


def ntt_pipe_plan(n_poly, L, n, chunk_bytes, k, min_chunks=1):
    """chunks on the busiest side stream of the transform's chunk schedule, 0: the caller's stream alone (moai_ntt_pipe_plan)"""
    return int(lib().moai_ntt_pipe_plan(n_poly, L, n, chunk_bytes, k, min_chunks))


def reset_tuning():
    """drop every set_tuning override: the environment's value, else the default, applies again"""
    _check(lib().moai_reset_tuning())


def op_trace(enable):
    """start (True: clears the counters) or stop the census of operations the entry points are asked to perform"""
    _check(lib().moai_op_trace(1 if enable else 0))


def op_trace_counts():
    """{(entry point, level): units} counted since op_trace(True)"""
    need = lib().moai_op_trace_dump(None, 0)
    buf = C.create_string_buffer(need + 16)
    lib().moai_op_trace_dump(buf, need + 16)
    out = {}
    for line in buf.value.decode().splitlines():
        name, level, count = line.split()
        out[(name, int(level))] = int(count)
    return out


def device_info(device=0):
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    hbm = sz(0)
    _check(lib().moai_device_info(device, name, 256, C.byref(cus), C.byref(hbm)))
    return name.value.decode(), cus.value, hbm.value


class Event:
    def __init__(self):
        p = vp()
        _check(lib().moai_event_create(C.byref(p)))
        self.ptr = p.value

    def record(self, stream=None):
        _check(lib().moai_event_record(self.ptr, stream))

    def elapsed_ms_since(self, start):
        ms = C.c_float(0)
        _check(lib().moai_event_elapsed_ms(start.ptr, self.ptr, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            lib().moai_event_destroy(self.ptr)
        except Exception:
            pass
