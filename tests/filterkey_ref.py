"""numpy restatement of the absence filter's key (aix_device.hpp: filter_key, bloom_word, bloom_mask) and, for comparison, of the key the
filter had before: Jenkins' lookup8 on the ASCII of the code, umul64hi(b, nwords), four 6-bit positions of c.

The filter is an open-time structure with no file format: one 64-bit word per key, chosen by `hw`, and one bit in each 16-bit quarter
of that word, chosen by four nibbles of `hb`. Everything here works on arrays of 46-bit codes (uint64)."""
import numpy as np

from aindex_amd import synth

_U32 = np.uint64(0xFFFFFFFF)
JENKINS_GOLDEN = np.uint64(0x9E3779B97F4A7C13)
OLD_KEY_SEED = 0x0123456789ABCDEF          # the comparison key's seed: any value serves, the MPHF's seed is a random number too


def _rot(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def filter_key(codes):
    """(hw, hb) as uint32 arrays: the final() of Bob Jenkins' lookup3 (public domain) over the two halves of the code"""
    codes = np.asarray(codes, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = (codes & _U32).astype(np.uint32) + np.uint32(0x9E3779B9)
        b = (codes >> np.uint64(32)).astype(np.uint32) + np.uint32(0x85EBCA6B)
        c = np.full(codes.shape, 0xC2B2AE35, dtype=np.uint32)
        c ^= b; c -= _rot(b, 14)
        a ^= c; a -= _rot(c, 11)
        b ^= a; b -= _rot(a, 25)
        c ^= b; c -= _rot(b, 16)
        a ^= c; a -= _rot(c, 4)
        b ^= a; b -= _rot(a, 14)
        c ^= b; c -= _rot(b, 24)
    return b, c


def word_index(hw, nwords):
    """__umulhi(hw, nwords)"""
    return ((hw.astype(np.uint64) * np.uint64(nwords)) >> np.uint64(32)).astype(np.int64)


def quarter_mask(hb):
    """one bit in each 16-bit quarter of the word, from the low 16 bits of hb"""
    h = hb.astype(np.uint64)
    one, f = np.uint64(1), np.uint64(15)
    return ((one << (h & f)) | (one << (np.uint64(16) + ((h >> np.uint64(4)) & f))) | (one << (np.uint64(32) + ((h >> np.uint64(8)) & f)))
            | (one << (np.uint64(48) + ((h >> np.uint64(12)) & f))))


def new_key(codes, nwords):
    hw, hb = filter_key(codes)
    return word_index(hw, nwords), quarter_mask(hb)


def _jmix(a, b, c):
    s = np.uint64
    for k1, k2, k3 in ((43, 9, 8), (38, 23, 5), (35, 49, 11), (12, 18, 22)):
        a -= b; a -= c; a ^= c >> s(k1)
        b -= c; b -= a; b ^= a << s(k2)
        c -= a; c -= b; c ^= b >> s(k3)
    return a, b, c


def jenkins23(codes, seed=OLD_KEY_SEED):
    """lookup8 (a, b, c) of the 23 ASCII bytes of each code"""
    asc = synth.decode_kmers(np.asarray(codes, dtype=np.uint64), 23)
    buf = np.zeros((asc.shape[0], 24), dtype=np.uint8)
    buf[:, :23] = asc
    w = buf.view("<u8")
    with np.errstate(over="ignore"):
        a = np.uint64(seed) + w[:, 0]
        b = np.uint64(seed) + w[:, 1]
        c = JENKINS_GOLDEN + np.uint64(23) + (w[:, 2] << np.uint64(8))
        return _jmix(a, b, c)


def old_key(codes, nwords, seed=OLD_KEY_SEED):
    """the key before: word = umul64hi(b, nwords), bits c & 63, (c >> 6) & 63, (c >> 12) & 63, (c >> 18) & 63"""
    _, b, c = jenkins23(codes, seed)
    n = np.uint64(nwords)                                                      # < 2^32, so the partial products fit 64 bits
    word = (((b >> np.uint64(32)) * n + (((b & _U32) * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)
    one, f = np.uint64(1), np.uint64(63)
    mask = (one << (c & f)) | (one << ((c >> np.uint64(6)) & f)) | (one << ((c >> np.uint64(12)) & f)) | (one << ((c >> np.uint64(18)) & f))
    return word, mask


def build_filter(word, mask, nwords):
    filt = np.zeros(nwords, dtype=np.uint64)
    np.bitwise_or.at(filt, word, mask)
    return filt


def passes(filt, word, mask):
    return (filt[word] & mask) == mask


def filter_words(nkeys, bits_per_key=16):
    """the handle's nbloom"""
    return int(nkeys * bits_per_key / 64.0) + 1


def canonical(codes):
    codes = np.asarray(codes, dtype=np.uint64)
    return np.minimum(codes, synth.revcomp_codes(codes, 23))


def neighbours(keys, n, k_seed=11, p_seed=12, b_seed=13):
    """n one-substitution neighbours of keys, canonical: key sm64(k_seed, i) % len(keys), base sm64(p_seed, i) % 23 (counted from the
    first base) xor-ed with sm64(b_seed, i) % 3 + 1"""
    i = np.arange(n, dtype=np.uint64)
    k = keys[(synth.sm64(k_seed, i) % np.uint64(keys.shape[0])).astype(np.int64)]
    pos = synth.sm64(p_seed, i) % np.uint64(23)
    x = synth.sm64(b_seed, i) % np.uint64(3) + np.uint64(1)
    return canonical(k ^ (x << (np.uint64(2) * (np.uint64(22) - pos))))
