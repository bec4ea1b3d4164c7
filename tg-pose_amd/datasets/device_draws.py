"""The host half of ``draws='device'`` (datasets/load_data.py): the counter-based generator of csrc/draws.hip restated in NumPy, bit
for bit, and the per-item scalar draws made from it.

A draw is a pure function of (seed, key, site, counter): ``philox_words`` are the four words of Philox-4x32-10 with Philox key (seed
low, seed high) and Philox counter (counter, site, key low, key high) -- what ``tgp_draw_words`` writes on the device
(tests/golden/device_draws.npz pins the two against each other).  The per-point draws and the permutations are made on the device
(sites 1-7 of include/tgpose.h); the per-item scalars that no device result feeds are made here from site 0, ``HOST_COUNTERS``
counters per item, laid out as ``ItemStream`` documents.  ``perm_at`` / ``perm_pos`` restate the device's permutation walk (tests).
"""
import numpy as np

from .. import _lib

HOST_COUNTERS = 64          # 256 words per item at site 0
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox_words(seed, keys, site, counters):
    """-> (len(keys), len(counters), 4) uint32: Philox-4x32-10 of every (key, counter) at ``site`` under ``seed``"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 1)
    ctr = np.asarray(counters, dtype=np.uint64).reshape(1, -1)
    seed = int(seed) & (2 ** 64 - 1)
    shape = (keys.shape[0], ctr.shape[1])
    c = [np.broadcast_to(ctr & _MASK, shape).copy(), np.full(shape, int(site), np.uint64), np.broadcast_to(keys & _MASK, shape).copy(),
         np.broadcast_to(keys >> np.uint64(32), shape).copy()]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]                # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform_f32(w):
    """torch.rand's float32 law: 24 bits, [0, 1)"""
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniform_f64(w0, w1):
    """NumPy's random_sample law: 53 bits, [0, 1)"""
    a = (np.asarray(w0, np.uint32) >> np.uint32(5)).astype(np.float64)
    b = (np.asarray(w1, np.uint32) >> np.uint32(6)).astype(np.float64)
    return (a * 67108864.0 + b) / 9007199254740992.0


# ------------------------------------------------------------------------------------------------- the permutation walk, restated
def _mix32(x):
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _MASK
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _MASK
    return x ^ (x >> np.uint64(16))


def half_bits_of(total):
    h = 1
    while (1 << (2 * h)) < total:
        h += 1
    return h


def feistel(v, h, key, inverse=False):
    """the keyed bijection of [0, 2^(2h)) (csrc/draws.hip feistel / feistel_inv) on an array of values"""
    v = np.asarray(v, dtype=np.uint64)
    mask = np.uint64((1 << h) - 1)
    l, r = v >> np.uint64(h), v & mask
    for rnd in (range(3, -1, -1) if inverse else range(4)):
        k = np.uint64((int(key) + 0x9e3779b9 * (rnd + 1)) & 0xFFFFFFFF)
        if inverse:
            l, r = r ^ (_mix32(l ^ k) & mask), l
        else:
            l, r = r, l ^ (_mix32(r ^ k) & mask)
    return (l << np.uint64(h)) | r


def _walk(v, total, key, inverse):
    h = half_bits_of(total)
    k = feistel(v, h, key, inverse)
    while True:
        out = k >= np.uint64(total)
        if not out.any():
            return k.astype(np.int64)
        k = np.where(out, feistel(k, h, key, inverse), k)


def perm_at(i, total, key):
    """element i of the permutation of [0, total) under the 32-bit Feistel key (cycle walking)"""
    return _walk(i, total, key, False)


def perm_pos(v, total, key):
    """the position of element v in that permutation"""
    return _walk(v, total, key, True)


def feistel_key(seed, key, site):
    """the 32-bit key of an item's permutation at ``site``: word 0 of counter 0"""
    return int(philox_words(seed, [key], site, [0])[0, 0, 0])


# ------------------------------------------------------------------------------------------------------- the per-item scalars
class ItemStream(object):
    """One item's site-0 words behind the few np.random methods the scalar draws call, so aug_bbox_dzi, generate_aug_parameters and
    the operators' ``draw`` run unchanged on it.  A float64 uniform takes two consecutive words (uniform_f64); ``seek`` moves to a
    named region so that a draw's words do not depend on how many an earlier draw took:
      words   0 ..  15   aug_bbox_DZI                 16 ..  17   defor_2D's rand()
      words  32 ..  63   generate_aug_parameters      64 ..  69   PC_BasicAugment's six float32 draws (one word each)
      word   70          the operator index (low two bits)
      words  72 .. 255   the operator's own scalars (skip test, dropout ratio, crop / cutout attempts)"""
    DZI, DEFOR, PARAMS, BASE, OP_INDEX, OPERATOR = 0, 16, 32, 64, 70, 72

    def __init__(self, words, doubles=None):
        self.w, self.at = words, 0
        self.d = uniform_f64(words[0::2], words[1::2]) if doubles is None else doubles       # pair j = words 2j, 2j + 1

    def seek(self, at):
        self.at = at
        return self

    def _doubles(self, n):
        if self.at + 2 * n > self.w.shape[0] or self.at % 2:
            raise ValueError("ItemStream: more scalar draws than HOST_COUNTERS provides (or an odd word offset)")
        j = self.at // 2
        self.at += 2 * n
        return self.d[j:j + n]

    def random_sample(self, size=None):
        if size is None:
            return float(self._doubles(1)[0])
        return self._doubles(int(np.prod(size))).reshape(size)

    def rand(self, *shape):
        return self.random_sample(shape if shape else None)

    def uniform(self, low=0.0, high=1.0, size=None):
        if size is None and isinstance(low, (int, float)) and isinstance(high, (int, float)):
            return low + (high - low) * self.random_sample()
        shape = np.broadcast(np.asarray(low), np.asarray(high)).shape if size is None else (size if isinstance(size, tuple) else (size,))
        if shape == ():
            return low + (high - low) * self.random_sample()
        return np.asarray(low) + (np.asarray(high) - np.asarray(low)) * self.random_sample(shape)

    def floats32(self, n):
        w = self.w[self.at:self.at + n]
        self.at += n
        return uniform_f32(w)

    def randint4(self):
        k = int(self.w[self.at] & np.uint32(3))
        self.at += 1
        return k


def item_streams(seed, keys):
    """one ItemStream per key"""
    w = philox_words(seed, keys, _lib.SITE_HOST, np.arange(HOST_COUNTERS)).reshape(len(keys), -1)
    dbl = uniform_f64(w[:, 0::2], w[:, 1::2])
    return [ItemStream(w[d], dbl[d]) for d in range(len(keys))]
