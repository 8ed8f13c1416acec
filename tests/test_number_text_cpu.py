"""The register-only number text of genomicsdb_amd/csrc/core/gdb_core.hpp (put_i64 / put_u32: packed digits, values above 2^32 split by
10^8) against Python's str(), and the single-pass ALT token iterator (AltTokens) against alt_token(idx), through tests/hostsim_numtext/.
The same comparisons run once more, against the C library, in a stand-alone program built with the address and undefined-behaviour
sanitizers.  put_float stays with tests/test_float_text.py."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import helpers

DIR = os.path.join(helpers.ROOT, "tests", "hostsim_numtext")

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        L = ctypes.CDLL(os.path.join(DIR, "libhostsim_numtext.so"))
        L.hostsim_numtext_put_i64.argtypes = [ctypes.c_int64, ctypes.c_char_p]
        L.hostsim_numtext_put_u32.argtypes = [ctypes.c_uint32, ctypes.c_char_p]
        L.hostsim_numtext_put_i64_many.restype = ctypes.c_int64
        L.hostsim_numtext_put_i64_many.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p]
        for f in (L.hostsim_numtext_alt_iterator, L.hostsim_numtext_alt_indexed):
            f.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        _lib = L
    return _lib


def i64_text(v):
    buf = ctypes.create_string_buffer(32)
    n = lib().hostsim_numtext_put_i64(v, buf)
    return buf.raw[:n].decode()


def u32_text(v):
    buf = ctypes.create_string_buffer(32)
    n = lib().hostsim_numtext_put_u32(v, buf)
    return buf.raw[:n].decode()


EDGES = [0, 1, -1, 9, 10, 99, 100, 10**8 - 1, 10**8, 10**8 + 1, 2**31 - 1, 2**32, 10**16 - 1, 10**16, 2**63 - 1, -2**63]


@pytest.mark.parametrize("v", EDGES)
def test_put_i64_edge_values(v):
    assert i64_text(v) == str(v)
    if -2**63 <= -v < 2**63:
        assert i64_text(-v) == str(-v)


def test_put_i64_random_values_of_every_digit_count():
    rng = random.Random(20240611)
    for digits in range(1, 20):
        lo, hi = (0 if digits == 1 else 10 ** (digits - 1)), min(10 ** digits - 1, 2**63 - 1)
        vals = [rng.randint(lo, hi) * (-1 if i & 1 else 1) for i in range(100000)]
        a = np.array(vals, dtype=np.int64)
        out = ctypes.create_string_buffer(22 * len(vals))
        n = lib().hostsim_numtext_put_i64_many(a.ctypes.data, len(vals), out)
        assert n > 0, "the counted length differs from the written one"
        assert out.raw[:n].decode() == "".join("%d\n" % v for v in vals), digits


@pytest.mark.parametrize("v", [0, 9, 10, 99, 100, 10**8 - 1, 10**8, 10**9 - 1, 10**9, 2**32 - 1])
def test_put_u32_edge_values(v):
    assert u32_text(v) == str(v)


def tokens(fn, s):
    off = (ctypes.c_int32 * 64)()
    ln = (ctypes.c_int32 * 64)()
    n = fn(s, len(s), off, ln, 64)
    assert 0 <= n <= 64
    return [(off[i], ln[i]) for i in range(n)]


def strtok_model(s):
    """(offset, length) of the non-empty '|' separated tokens"""
    out, i = [], 0
    for part in s.split(b"|"):
        if part:
            out.append((i, len(part)))
        i += len(part) + 1
    return out


ALTS = [b"", b"|", b"A", b"A|", b"|A", b"A||C", b"&", b"A|&", b"||"]


@pytest.mark.parametrize("s", ALTS)
def test_token_iterator_on_the_edge_strings(s):
    L = lib()
    assert tokens(L.hostsim_numtext_alt_iterator, s) == tokens(L.hostsim_numtext_alt_indexed, s) == strtok_model(s)


def test_token_iterator_on_random_strings():
    L = lib()
    rng = random.Random(77)
    for _ in range(10000):
        s = bytes(rng.choice(b"AC|&*<>") for _ in range(rng.randrange(0, 24)))
        it = tokens(L.hostsim_numtext_alt_iterator, s)
        assert it == tokens(L.hostsim_numtext_alt_indexed, s), s
        assert it == strtok_model(s), s


def test_stand_alone_program_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", DIR])
    r = subprocess.run([os.path.join(DIR, "hostsim_numtext_main")], capture_output=True, text=True)
    assert r.returncode == 0 and "ok: 0 mismatches" in r.stdout, r.stdout + r.stderr
