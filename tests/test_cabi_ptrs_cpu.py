"""CPU-only checks of the key switches on a list of ciphertexts (moai_apply_galois_ptrs, moai_relinearize_ptrs): both are
exported and bound, their header comments cite the reference, and the arguments that need no context -- an empty list, a
null list or member, an even Galois element -- are answered before the device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
NAMES = ("moai_apply_galois_ptrs", "moai_relinearize_ptrs")
vp = C.c_void_p


def test_symbols_exported_and_declared(moai):
    L = C.CDLL(moai.lib_path())
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in moai.hip.SYMBOLS, name
    assert callable(moai.Context.apply_galois_ptrs) and callable(moai.Context.relinearize_ptrs)


def test_header_comments_cite_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "moai_hip.h")).read()
    for name in NAMES:
        at = hdr.index("int " + name + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert comment.rstrip().endswith("*/"), name  # the comment sits directly on the declaration
        assert re.search(r"SEAL/evaluator\.cpp:\d+-\d+", comment), name


def test_arguments_refused_without_a_device(moai):
    lib = moai.hip.lib()
    gal, rel = lib.moai_apply_galois_ptrs, lib.moai_relinearize_ptrs
    blk = (vp * 2)(0x1000, 0x2000)  # never dereferenced: every call below returns before it reaches the context
    out = (vp * 2)(0x3000, 0x4000)
    hole = (vp * 2)(0x1000, None)
    odd, even = (C.c_uint32 * 2)(3, 5), (C.c_uint32 * 2)(3, 6)
    # n == 0 is MOAI_OK whatever else is passed
    assert gal(None, None, None, 3, None, None, None, 0, None) == OK
    assert rel(None, None, None, None, 3, 0, None) == OK
    # null lists
    for args in ((None, None, out, 3, odd, blk, None, 2, None), (None, blk, None, 3, odd, blk, None, 2, None),
                 (None, blk, out, 3, None, blk, None, 2, None), (None, blk, out, 3, odd, None, None, 2, None)):
        assert gal(*args) == EINVAL and b"null list" in lib.moai_last_error(), args
    for args in ((None, None, out, 0x5000, 3, 2, None), (None, blk, None, 0x5000, 3, 2, None), (None, blk, out, None, 3, 2, None)):
        assert rel(*args) == EINVAL and b"null list" in lib.moai_last_error(), args
    # a null member, named
    assert gal(None, hole, out, 3, odd, blk, None, 2, None) == EINVAL and b"member 1: null pointer" in lib.moai_last_error()
    assert gal(None, blk, hole, 3, odd, blk, None, 2, None) == EINVAL and b"member 1: null pointer" in lib.moai_last_error()
    assert gal(None, blk, out, 3, odd, hole, None, 2, None) == EINVAL and b"member 1: null pointer" in lib.moai_last_error()
    assert rel(None, hole, out, 0x5000, 3, 2, None) == EINVAL and b"member 1: null pointer" in lib.moai_last_error()
    # an even element, named
    assert gal(None, blk, out, 3, even, blk, None, 2, None) == EINVAL
    assert b"member 1: Galois element is not valid" in lib.moai_last_error()
    # with valid lists the missing context is what is reported
    assert gal(None, blk, out, 3, odd, blk, None, 2, None) == EINVAL and b"null context" in lib.moai_last_error()
    assert rel(None, blk, out, 0x5000, 3, 2, None) == EINVAL and b"null context" in lib.moai_last_error()
