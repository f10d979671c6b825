"""encode23_clean (aix_device.hpp: the encoder of pass A of the binned lookup, which drops a query with other bytes) against
encode23_words on the host: a small program built with the project's hipcc, host side only, that includes aix_device.hpp and compares
the two on seeded random strings, on every byte value at every position of clean k-mers and on a few fixed k-mers. `valid` must agree
everywhere and the code wherever `valid` holds. No GPU."""
import os
import subprocess

import pytest

from aindex_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(_lib.ROOT, "aindex_amd", "csrc")

SRC = r"""
#include <cstdio>
#include <cstring>
#include "aix_device.hpp"

static uint64_t sm64(uint64_t& s) {                          // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static unsigned long long n_all = 0, n_valid = 0, n_bad = 0;
// the words load23 makes of the 23 bytes, and the same words with a 24th byte that is not the query's
static void check(const uint8_t* s, uint8_t byte24) {
    uint8_t b[24];
    memcpy(b, s, 23);
    b[23] = byte24;
    uint64_t w0, w1, w2;
    memcpy(&w0, b, 8); memcpy(&w1, b + 8, 8); memcpy(&w2, b + 16, 8);
    const aix::Enc23 e = aix::encode23_words(w0, w1, w2);
    uint64_t code = ~0ull;
    const bool v = aix::encode23_clean(w0, w1, w2, code);
    ++n_all;
    n_valid += e.valid;
    if (v != e.valid || (v && code != e.code)) {
        if (n_bad++ < 10) printf("MISMATCH %.23s byte24=%u valid %d/%d code %llx/%llx\n", (const char*)s, byte24, (int)e.valid, (int)v,
                                 (unsigned long long)e.code, (unsigned long long)code);
    }
}
int main() {
    const char* alpha = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTacgtNnU*@-";
    const int na = (int)strlen(alpha);
    uint64_t seed = 20240607;
    uint8_t s[23];
    // 2^20 seeded strings over an alphabet weighted towards ACGT (120 of 130 letters), every eighth with one uniformly random byte
    unsigned long long rand_valid = 0;
    for (int it = 0; it < (1 << 20); ++it) {
        for (int j = 0; j < 23; ++j) s[j] = (uint8_t)alpha[sm64(seed) % (uint64_t)na];
        if ((it & 7) == 7) s[sm64(seed) % 23] = (uint8_t)sm64(seed);
        const unsigned long long before = n_valid;
        check(s, 0);
        check(s, (uint8_t)sm64(seed));
        rand_valid += n_valid - before;
    }
    // every byte value at every position of eight clean k-mers
    for (int k = 0; k < 8; ++k) {
        uint8_t base[23];
        for (int j = 0; j < 23; ++j) base[j] = (uint8_t)"ACGT"[sm64(seed) & 3];
        for (int pos = 0; pos < 23; ++pos)
            for (int v = 0; v < 256; ++v) {
                memcpy(s, base, 23);
                s[pos] = (uint8_t)v;
                check(s, 0);
                check(s, (uint8_t)v);
            }
    }
    // all-A, all-C, all-G, all-T, alternating
    for (const char* fixed : {"AAAAAAAAAAAAAAAAAAAAAAA", "CCCCCCCCCCCCCCCCCCCCCCC", "GGGGGGGGGGGGGGGGGGGGGGG", "TTTTTTTTTTTTTTTTTTTTTTT",
                              "ACACACACACACACACACACACA", "TGTGTGTGTGTGTGTGTGTGTGT", "ATATATATATATATATATATATA", "CGCGCGCGCGCGCGCGCGCGCGC"}) {
        const unsigned long long before = n_valid;
        check((const uint8_t*)fixed, 0);
        check((const uint8_t*)fixed, 0xFF);
        if (n_valid - before != 2) { printf("fixed k-mer %s is not valid\n", fixed); ++n_bad; }
    }
    uint64_t code = 0;
    uint64_t w0, w1, w2 = 0;
    memcpy(&w0, "TTTTTTTT", 8); memcpy(&w1, "TTTTTTTT", 8); memcpy(&w2, "TTTTTTT", 7);
    if (!aix::encode23_clean(w0, w1, w2, code) || code != (1ull << 46) - 1) { printf("all-T code %llx\n", (unsigned long long)code); ++n_bad; }
    printf("checked %llu valid %llu random_valid %llu bad %llu\n", n_all, n_valid, rand_valid, n_bad);
    return n_bad ? 1 : 0;
}
"""


def test_clean_encoder_equals_encode23_words(tmp_path):
    src = tmp_path / "lb_encode_check.cpp"
    src.write_text(SRC)
    exe = tmp_path / "lb_encode_check"
    # host side only: the device pass is skipped, so the helpers' host fallbacks (lut4's loop, dot4's loop) are what runs
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", f"-I{CSRC}", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    last = out.strip().split("\n")[-1].split()
    checked, valid, rand_valid, bad = int(last[1]), int(last[3]), int(last[5]), int(last[7])
    assert bad == 0 and checked == 2 * ((1 << 20) + 8 * 23 * 256 + 8)
    # both outcomes are well represented among the random strings: (120/130)^23 = 16 % of those left alone are clean
    assert 2 * 100_000 < rand_valid < 2 * 250_000
    # of the 256 values at a position exactly four keep a k-mer clean
    assert valid - rand_valid == 2 * (8 * 23 * 4 + 8)
