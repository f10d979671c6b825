"""bloom_fold / bloom_fold_test (aix_device.hpp: the one-byte coarse image of a filter word that pass B of the binned lookup tests in
LDS) against bloom_mask on the host: a small program built with the project's hipcc, host side only. On random words of every
density and random and exhaustive keys: a word that passes the full mask of hb has coarse bit hb & 7 set, a word whose coarse bit is
clear never passes, and the image of a word depends on its quarter 0 alone. No GPU."""
import os
import subprocess

from aindex_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(_lib.ROOT, "aindex_amd", "csrc")

SRC = r"""
#include <cstdio>
#include "aix_device.hpp"

static uint64_t sm64(uint64_t& s) {                          // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static unsigned long long n_all = 0, n_pass = 0, n_clear = 0, n_bad = 0;
static void check(uint64_t word, uint32_t hb) {
    const uint64_t m = aix::bloom_mask(hb);
    const bool pass = (word & m) == m, coarse = aix::bloom_fold_test(aix::bloom_fold(word), hb);
    ++n_all;
    n_pass += pass;
    n_clear += !coarse;
    if ((pass && !coarse) || aix::bloom_fold(word) > 0xFFu || aix::bloom_fold(word) != aix::bloom_fold(word & 0xFFFFull)) {
        if (n_bad++ < 10) printf("MISMATCH word %llx hb %x pass %d coarse %d\n", (unsigned long long)word, hb, (int)pass, (int)coarse);
    }
}
int main() {
    uint64_t seed = 20240911;
    // words of k keys each, k = 0 .. 15 (the filter holds four on average), and words of random bits thinned by 0 .. 3 ands
    for (int it = 0; it < (1 << 18); ++it) {
        uint64_t word = 0;
        const int k = it & 15;
        uint32_t keys[16];
        for (int j = 0; j < k; ++j) word |= aix::bloom_mask(keys[j] = (uint32_t)sm64(seed));
        check(word, (uint32_t)sm64(seed));                      // any key
        if (k) {                                                // a key of the word
            const unsigned long long before = n_pass;
            check(word, keys[(it >> 4) % k]);
            if (n_pass == before) { printf("own key does not pass\n"); ++n_bad; }
        }
        uint64_t thin = sm64(seed);
        for (int j = 0; j < (it >> 4 & 3); ++j) thin &= sm64(seed);
        check(thin, (uint32_t)sm64(seed));
    }
    // every value of the 16 bits the mask reads, against a word of one key and against its complement
    for (uint32_t hb = 0; hb < 65536; ++hb) {
        const uint64_t own = aix::bloom_mask(hb);
        check(own, hb);
        check(~own, hb);
        check(own, hb ^ 1u);
        check(own, hb ^ 8u);                                    // the other bit of quarter 0 that folds onto the same image bit
        if (aix::bloom_fold(own) != (1u << (hb & 7)) || !aix::bloom_fold_test(aix::bloom_fold(own), hb ^ 8u) || aix::bloom_fold_test(aix::bloom_fold(own), hb ^ 1u)) {
            printf("image of the word of key %x is %x\n", hb, aix::bloom_fold(own));
            ++n_bad;
        }
    }
    printf("checked %llu pass %llu clear %llu bad %llu\n", n_all, n_pass, n_clear, n_bad);
    return n_bad ? 1 : 0;
}
"""


def test_fold_never_hides_a_passing_word(tmp_path):
    src = tmp_path / "lb_fold_check.cpp"
    src.write_text(SRC)
    exe = tmp_path / "lb_fold_check"
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", f"-I{CSRC}", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    last = out.strip().split("\n")[-1].split()
    checked, passed, clear, bad = int(last[1]), int(last[3]), int(last[5]), int(last[7])
    assert bad == 0
    assert checked == (1 << 18) * 2 + (1 << 18) * 15 // 16 + 4 * 65536
    # both outcomes are well represented: the own keys and the 65 536 one-key words pass, and far more words have the coarse bit clear
    assert passed >= (1 << 18) * 15 // 16 + 65536 and clear > 65536 * 2
