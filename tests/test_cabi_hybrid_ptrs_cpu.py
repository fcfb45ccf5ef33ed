"""CPU-only checks of the hybrid key switches on a list of ciphertexts (include/moai_hip.h, "hybrid key switches on a list of
ciphertexts": moai_apply_galois_hybrid_to, moai_apply_galois_hybrid_acc, moai_apply_galois_hybrid_ptrs, moai_relinearize_hybrid_ptrs,
moai_relinearize_rescale_hybrid_ptrs):
(a) the five symbols are exported, declared, bound and in SYMBOLS;
(b) each header comment sits on its declaration and cites the reference lines of the function it stands for;
(c) the refusals that need no device arrive in the documented order, with a null context and pointers that are never dereferenced."""
import ctypes as C
import re

from hybrid_kit import EINVAL, OK, exported, header, header_comment

# name -> (the Context method, what its comment cites besides switch_key_inplace)
NAMES = {
    "moai_apply_galois_hybrid_to": ("apply_galois_hybrid_to", ["SEAL/evaluator.cpp:2563-2665"]),
    "moai_apply_galois_hybrid_acc": ("apply_galois_hybrid_acc", ["SEAL/evaluator.cpp:2563-2665"]),
    "moai_apply_galois_hybrid_ptrs": ("apply_galois_hybrid_ptrs", ["SEAL/evaluator.cpp:2563-2665"]),
    "moai_relinearize_hybrid_ptrs": ("relinearize_hybrid_ptrs", ["SEAL/evaluator.cpp:1345-1400"]),
    "moai_relinearize_rescale_hybrid_ptrs": ("relinearize_rescale_hybrid_ptrs", ["SEAL/evaluator.cpp:1345-1400", "Evaluator::rescale_to_next"]),
}


def test_symbols_exported_declared_and_bound(moai):
    exported(moai, NAMES, [method for method, _ in NAMES.values()])
    hdr = header()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name


def test_section_follows_relinearize_rescale():
    hdr = header()
    at = hdr.index("/* ---- hybrid key switches on a list of ciphertexts")
    assert hdr.index("/* ---- hybrid relinearize + rescale") < at < hdr.index("/* ---- stream audit")
    for name in NAMES:
        assert hdr.index("int " + name + "(") > at, name


def test_header_comments_cite_reference_lines():
    for name, (_, cites) in NAMES.items():
        comment = header_comment(name)
        assert re.search(r"SEAL/evaluator\.cpp:\d+-\d+", comment), name
        assert "SEAL/evaluator.cpp:2724-3020" in comment, name  # switch_key_inplace
        for cite in cites:
            assert cite in comment, (name, cite)


def test_list_refusals_arrive_in_order_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000  # never dereferenced: every call below returns before it reaches a device pointer or the context
    vp = C.c_void_p

    def ptrs(*v):
        return (vp * len(v))(*v)

    def elts(*v):
        return (C.c_uint32 * len(v))(*v)

    good, hole = ptrs(p, p), ptrs(p, None)
    odd, even = elts(3, 5), elts(3, 4)

    def galois(ins=good, outs=good, L=3, alpha=2, e=odd, keys=good, n=2):
        return lib.moai_apply_galois_hybrid_ptrs(None, ins, outs, L, alpha, e, keys, None, n, None)

    def relin(fn):
        return lambda ins=good, outs=good, L=3, alpha=2, key=p, n=2: fn(None, ins, outs, key, L, alpha, n, None)

    def refused(rc, msg):
        assert rc == EINVAL and msg in lib.moai_last_error(), (rc, msg, lib.moai_last_error())

    # 1. n == 0 is MOAI_OK whatever else is passed
    assert galois(ins=None, outs=None, L=0, alpha=0, e=None, keys=None, n=0) == OK
    # 2. a null list, before any member and before alpha and L
    for kw in (dict(ins=None), dict(outs=None), dict(e=None), dict(keys=None)):
        refused(galois(L=0, alpha=0, **kw), b"null list")
    # 3. a null member or an even element, by member, before alpha and L
    for kw in (dict(ins=hole), dict(outs=hole), dict(keys=hole)):
        refused(galois(L=0, alpha=0, **kw), b"member 1: null pointer")
    refused(galois(L=0, alpha=0, e=even), b"member 1: Galois element is not valid")
    refused(galois(ins=hole, e=even), b"member 1: null pointer")
    # 4. hy_check's order: alpha = 0, L = 0, then the context
    refused(galois(L=0, alpha=0), b"alpha = 0")
    refused(galois(L=0), b"L = 0")
    refused(galois(), b"null context")

    for fn in (lib.moai_relinearize_hybrid_ptrs, lib.moai_relinearize_rescale_hybrid_ptrs):
        call = relin(fn)
        assert call(ins=None, outs=None, L=0, alpha=0, key=None, n=0) == OK
        for kw in (dict(ins=None), dict(outs=None), dict(key=None)):
            refused(call(L=0, alpha=0, **kw), b"null list")
        for kw in (dict(ins=hole), dict(outs=hole)):
            refused(call(L=0, alpha=0, **kw), b"member 1: null pointer")
        refused(call(L=0, alpha=0), b"alpha = 0")
        refused(call(L=0), b"L = 0")
        refused(call(), b"null context")
    # the rescale form needs L >= 2 and alpha + 1 <= 16, in moai_relinearize_rescale_hybrid's words and place
    call = relin(lib.moai_relinearize_rescale_hybrid_ptrs)
    refused(call(L=1, alpha=0), b"alpha = 0")
    refused(call(L=1), b"L = 1: no prime left to rescale to")
    refused(call(alpha=16), b"alpha = 16")
    refused(relin(lib.moai_relinearize_hybrid_ptrs)(L=1), b"null context")


def test_to_and_acc_refusals_without_a_device(moai):
    lib = moai.hip.lib()
    p = 0x1000
    for fn in (lib.moai_apply_galois_hybrid_to, lib.moai_apply_galois_hybrid_acc):
        # moai_apply_galois_hybrid's order: an even element, alpha = 0, L = 0, then the context
        for L, alpha, elt, msg in ((0, 0, 4, b"Galois element is not valid"), (0, 0, 3, b"alpha = 0"), (0, 2, 3, b"L = 0"), (3, 2, 3, b"null context")):
            assert fn(None, p, p + 8, L, alpha, elt, p, 1, None) == EINVAL
            assert msg in lib.moai_last_error(), (L, alpha, elt, lib.moai_last_error())
