"""Directed operands for the software x87 (openshmem-async_amd/csrc/ld80.h)
and the Annex G complex product (cmul in fold_ops.h): numpy only, no torch,
no GPU.

pairs() builds named groups of (a, b) 80-bit encodings, fixed seed, as 16-byte
slots viewed as np.longdouble: every alignment distance of the fast add with
ties, sticky bits and carries, at mid-range exponents, at the overflow boundary
and at the underflow boundary; the general add on denormals and
pseudo-denormals; products over the whole denormal range and the overflow
boundary, with ties, carries and exact results; NaNs, unsupported encodings and
invalid operations; the comparisons of min and max.  third() derives a third
operand from the host's own a op b for the three-input routes.

census() classifies a pair by the path it must take.  It is written with
Python integers from the format's definition (Intel SDM vol. 1, 4.8 and 8.2),
not from ld80.h, and computes the correctly rounded sum and product on the
way, so it is also a second reference beside the host's x87.  cover() picks a
small sublist that still holds every census class.

annex_g_operands() builds the operands of the complex-product tests.
"""
from collections import Counter

import numpy as np

BIAS = 16383
EMAX = 0x7FFE
TOP = 1 << 63
ALL = (1 << 64) - 1
QUIET = 1 << 62
MAX_PAIRS = 1 << 16           # 1 MiB per operand
SIGNS = ((0, 0), (0, 1), (1, 0), (1, 1))
DMAX = 70
MUL_LOW = range(-66, 3)       # raw biased exponent of a product: the denormal range and around it
MUL_HIGH = range(0x7FFD, 0x8001)


# ------------------------------------------------------------------ encodings
def enc(neg, e, sig):
    """One encoding as (sig, sign | exponent)."""
    assert 0 <= e <= 0x7FFF and 0 <= sig <= ALL
    return (sig, (0x8000 if neg else 0) | e)


def to_slots(encs):
    """[(sig, se), ...] as np.longdouble (16-byte slots, padding zero)."""
    raw = np.zeros((len(encs), 2), dtype=np.uint64)
    if encs:
        raw[:, 0] = np.array([s for s, _ in encs], dtype=np.uint64)
        raw[:, 1] = np.array([se for _, se in encs], dtype=np.uint64)
    return raw.view(np.longdouble).reshape(len(encs))


def from_slots(x):
    """np.longdouble array as [(sig, se), ...] of Python integers."""
    raw = np.ascontiguousarray(x).view(np.uint64).reshape(-1, 2)
    return [(int(s), int(se) & 0xFFFF) for s, se in raw]


def classify(v):
    sig, se = v
    e = se & 0x7FFF
    if e == 0:
        return "zero" if sig == 0 else "pseudo-denormal" if sig & TOP else "denormal"
    if not sig & TOP:
        return "unnormal" if e != 0x7FFF else "pseudo-inf" if sig == 0 else "pseudo-nan"
    if e != 0x7FFF:
        return "normal"
    if sig == TOP:
        return "inf"
    return "qnan" if sig & QUIET else "snan"


UNSUPPORTED = ("unnormal", "pseudo-inf", "pseudo-nan")
FINITE = ("zero", "denormal", "pseudo-denormal", "normal")
INDEFINITE = enc(1, 0x7FFF, TOP | QUIET)


# ------------------------------------------- exact arithmetic, Python integers
def _exact(v):
    """A finite supported encoding as (signed integer m, q): value m * 2^q."""
    sig, se = v
    m = -sig if se & 0x8000 else sig
    return m, max(se & 0x7FFF, 1) - BIAS - 63


def _round(neg, M, q):
    """M * 2^q (M > 0) rounded to nearest even into the format.  Returns the
    encoding and the facts of the rounding: how (exact / inexact / tie), the
    parity of the kept significand before rounding, whether rounding carried
    out of the significand, and the biased exponent the unrounded value has
    when written with a 64-bit significand (below 1: the denormal range)."""
    shift = M.bit_length() - 64
    E = q + shift + 63 + BIAS
    raw = E
    if E < 1:
        shift += 1 - E
        E = 1
    how, parity, carry = "exact", None, False
    if shift <= 0:
        sig = M << -shift
    else:
        sig, rem, half = M >> shift, M & ((1 << shift) - 1), 1 << (shift - 1)
        parity = sig & 1
        if rem:
            how = "tie" if rem == half else "inexact"
        if rem > half or (rem == half and parity):
            sig += 1
            if sig > ALL:
                sig, E, carry = TOP, E + 1, True
    if E > EMAX:
        return enc(neg, 0x7FFF, TOP), how, parity, carry, raw
    return enc(neg, E if sig & TOP else 0, sig), how, parity, carry, raw


def _nan_result(a, b, ca, cb):
    """x87 rule for NaN operands: quiet beats signalling, then the larger
    significand, then the positive one; the result is quieted."""
    an, bn = ca in ("qnan", "snan"), cb in ("qnan", "snan")
    if an and bn:
        if ca != cb:
            r = a if ca == "qnan" else b
        elif a[0] != b[0]:
            r = a if a[0] > b[0] else b
        else:
            r = b if a[1] & 0x8000 else a
    else:
        r = a if an else b
    return (r[0] | QUIET, r[1])


def _result_class(r):
    c = classify(r)
    return {"qnan": "nan", "snan": "nan", "pseudo-denormal": "normal"}.get(c, c)


def exact_add(a, b):
    """(result encoding, labels) of a + b."""
    ca, cb = classify(a), classify(b)
    if ca in UNSUPPORTED or cb in UNSUPPORTED:
        return INDEFINITE, ["add:invalid"]
    if "nan" in ca or "nan" in cb:
        return _nan_result(a, b, ca, cb), ["add:nan-operand"]
    sa, sb = a[1] >> 15, b[1] >> 15
    if ca == "inf" or cb == "inf":
        if ca == cb:
            return (a, ["add:inf"]) if sa == sb else (INDEFINITE, ["add:invalid"])
        return (a if ca == "inf" else b), ["add:inf"]
    labels = []
    if ca == cb == "normal":
        d = abs((a[1] & 0x7FFF) - (b[1] & 0x7FFF))
        labels.append("add:d=%s:%s%s" % (d if d <= DMAX else "far", "+-"[sa], "+-"[sb]))
    (ma, qa), (mb, qb) = _exact(a), _exact(b)
    q = min(qa, qb)
    S = (ma << (qa - q)) + (mb << (qb - q))
    if S == 0:
        zero_sign = sa and sb if ca == cb == "zero" else 0
        return enc(zero_sign, 0, 0), labels + ["add:exact", "add:" + ("zeros" if ca == cb == "zero" else "cancel")]
    r, how, parity, carry, _ = _round(S < 0, abs(S), q)
    labels.append("add:" + how + ("" if how != "tie" else ":odd" if parity else ":even"))
    if carry:
        labels.append("add:round-carry")
    if classify(r) == "inf":
        labels.append("add:overflow")
    if ca == cb == "normal" and classify(r) == "denormal":
        labels.append("add:cancel-into-denormal")
    if ca != "normal" or cb != "normal":
        labels.append("add:general:%s,%s" % (ca, cb))
    return r, labels


def exact_mul(a, b):
    """(result encoding, labels) of a * b."""
    ca, cb = classify(a), classify(b)
    if ca in UNSUPPORTED or cb in UNSUPPORTED:
        return INDEFINITE, ["mul:invalid"]
    if "nan" in ca or "nan" in cb:
        return _nan_result(a, b, ca, cb), ["mul:nan-operand"]
    neg = (a[1] >> 15) != (b[1] >> 15)
    if ca == "inf" or cb == "inf":
        if ca == "zero" or cb == "zero":
            return INDEFINITE, ["mul:invalid"]
        return enc(neg, 0x7FFF, TOP), ["mul:inf"]
    if ca == "zero" or cb == "zero":
        return enc(neg, 0, 0), ["mul:exact", "mul:zero-operand"]
    (ma, qa), (mb, qb) = _exact(a), _exact(b)
    r, how, parity, carry, raw = _round(neg, abs(ma * mb), qa + qb)
    # a tie among normals is the fast path's own rounding; one made by
    # denormalising is the general path's
    tie = ("tie" if raw >= 1 else "tie-denormal") + (":odd" if parity else ":even")
    labels = ["mul:" + (tie if how == "tie" else how)]
    if carry:
        labels.append("mul:round-carry")
    if raw in MUL_LOW or raw in MUL_HIGH:
        labels.append("mul:e=%d" % raw)
    if classify(r) == "inf":
        labels.append("mul:overflow")
    if ca != "normal" or cb != "normal":
        labels.append("mul:general:%s,%s" % (ca, cb))
    return r, labels


def exact_less(a, b):
    """a < b as fucomip decides it: unordered is false, -0 == +0."""
    ca, cb = classify(a), classify(b)
    if ca in UNSUPPORTED or cb in UNSUPPORTED or "nan" in ca or "nan" in cb:
        return False
    def key(v, c):
        if c == "inf":
            return (-1 if v[1] & 0x8000 else 1, 0, 0)
        m, q = _exact(v)
        return (0, m, q)
    (ia, ma, qa), (ib, mb, qb) = key(a, ca), key(b, cb)
    if ia or ib:
        return ia < ib
    q = min(qa, qb)
    return (ma << (qa - q)) < (mb << (qb - q))


def census(a, b):
    """Per pair of the np.longdouble arrays a, b: (labels, sum, product, a < b,
    a > b), labels a tuple of strings naming the paths the pair must take:
    the operand classes, for add the exponent distance and signs, tie (with
    parity) / inexact / exact, rounding carry, overflow, cancellation into the
    denormal range, and the result's class; the same for mul with the raw
    result exponent around the denormal range and the overflow boundary."""
    out = []
    for x, y in zip(from_slots(a), from_slots(b)):
        s, ls = exact_add(x, y)
        p, lp = exact_mul(x, y)
        labels = ["cls:%s,%s" % (classify(x), classify(y))] + ls + lp
        labels += ["add:res=" + _result_class(s), "mul:res=" + _result_class(p)]
        lt, gt = exact_less(x, y), exact_less(y, x)
        labels.append("cmp:" + ("lt" if lt else "gt" if gt else "neither"))
        out.append((tuple(labels), s, p, lt, gt))
    return out


def counts(cen, idx=None):
    """How many pairs carry each label (of the pairs idx, default all)."""
    c = Counter()
    for i in (range(len(cen)) if idx is None else idx):
        c.update(cen[i][0])
    return c


def cover(cen, groups=None):
    """Indices of a small sublist that holds every census label (and, with
    groups, every group) of the whole list at least once: greedy set cover,
    in index order among equals, so it is the same list every time."""
    sets = [set(c[0]) | ({"grp:" + groups[i]} if groups is not None else set()) for i, c in enumerate(cen)]
    need = set().union(*sets) if sets else set()
    owners = {}
    for i, s in enumerate(sets):
        for lab in s:
            owners.setdefault(lab, []).append(i)
    picked = []
    gain = [len(s) for s in sets]
    while need:
        i = max(range(len(sets)), key=lambda k: (gain[k], -k))
        picked.append(i)
        for lab in sets[i] & need:
            for k in owners[lab]:
                gain[k] -= 1
        need -= sets[i]
    return sorted(picked)


# ------------------------------------------------------------------- the list
class _List:
    def __init__(self):
        self.a, self.b, self.groups = [], [], []

    def add(self, group, x, y):
        self.a.append(x)
        self.b.append(y)
        self.groups.append(group)

    def both(self, group, x, y):
        """(x, y) as group/ab and (y, x) as group/ba."""
        self.add(group + "/ab", x, y)
        self.add(group + "/ba", y, x)


def _add_normals(L, rng, group, exp_a, opposite_only=False):
    """Every d in 0..70, every sign combination, eight variants; exp_a(d, k)
    is a's exponent, b's is d below it."""
    def r64():
        return int(rng.integers(0, 1 << 64, dtype=np.uint64)) | TOP
    for d in range(DMAX + 1):
        for sa, sb in SIGNS:
            if opposite_only and sa == sb:
                continue
            x = r64()
            variants = [
                (r64(), r64()),                       # random significands
                (x, x ^ int(rng.integers(0, 8))),     # nearly equal
                (r64() & ~1, TOP),                    # d = 64: a tie, kept significand even
                (r64() | 1, TOP),                     # d = 64: a tie, kept significand odd
                (r64(), TOP | 1),                     # d = 65: sticky from bit 0 alone
                (ALL, r64()),                         # rounding carries out of the significand
                (ALL, TOP),                           # the same on a tie
                (TOP, ALL),                           # a power of two less nearly an ulp
            ]
            for k, (ma, mb) in enumerate(variants):
                ea = exp_a(d, k)
                L.add(group, enc(sa, ea, ma), enc(sb, ea - d, mb))


def _representatives(rng):
    """A few encodings of every class, both signs of each."""
    def r64():
        return int(rng.integers(0, 1 << 64, dtype=np.uint64))
    reps = []
    for neg in (0, 1):
        reps += [
            enc(neg, 0, 0),                                  # zero
            enc(neg, 0, 1),                                  # the smallest denormal
            enc(neg, 0, TOP - 1),                            # the largest denormal
            enc(neg, 0, r64() >> 7),                         # a denormal
            enc(neg, 0, TOP),                                # pseudo-denormal: the smallest normal's value
            enc(neg, 0, r64() | TOP),                        # a pseudo-denormal
            enc(neg, 1, TOP),                                # the smallest normal
            enc(neg, 40, r64() | TOP),                       # a small normal
            enc(neg, BIAS, TOP),                             # 1.0
            enc(neg, BIAS + 1, r64() | TOP),                 # a normal
            enc(neg, EMAX, ALL),                             # the largest finite
            enc(neg, 0x7FFF, TOP),                           # infinity
            enc(neg, 0x7FFF, TOP | QUIET),                   # quiet NaN, payload 0 (-: real indefinite)
            enc(neg, 0x7FFF, TOP | QUIET | 0x1234),          # quiet NaN, a payload
            enc(neg, 0x7FFF, TOP | 0x1234),                  # signalling NaN, the same payload
            enc(neg, 0x7FFF, TOP | 1),                       # signalling NaN, the smallest payload
            enc(neg, 0x7FFF, TOP | (QUIET - 1)),             # signalling NaN, the largest payload
            enc(neg, 0x7FFF, ALL),                           # quiet NaN, the largest payload
            enc(neg, 0x7FFF, 0),                             # pseudo-infinity
            enc(neg, 0x7FFF, QUIET | 5),                     # pseudo-NaN
            enc(neg, BIAS, 0),                               # unnormal, significand 0
            enc(neg, BIAS + 3, r64() >> 1),                  # unnormal
            enc(neg, 1, TOP - 1),                            # unnormal beside the largest denormal
        ]
    return reps


def _build():
    rng = np.random.default_rng(0x87ED6E5)
    L = _List()

    def r64():
        return int(rng.integers(0, 1 << 64, dtype=np.uint64))

    # ---- add, both operands normal
    _add_normals(L, rng, "add/normal/mid", lambda d, k: BIAS - 3 + (d + k) % 7 + d // 2)
    _add_normals(L, rng, "add/normal/top", lambda d, k: EMAX)
    _add_normals(L, rng, "add/normal/low", lambda d, k: d + 1 + k % 3)
    # cancellation of normals into the denormal range: equal exponents 1..70,
    # significands that differ in one low bit or a low field; and one
    # exponent apart (2^63 against nearly 2^64 one below)
    for e in range(1, 71):
        x = r64() | TOP
        k = int(rng.integers(0, min(63, max(1, 64 - e) + 8)))
        for sa, sb in ((0, 1), (1, 0)):
            L.add("add/cancel-into-denormal", enc(sa, e, x), enc(sb, e, x ^ (1 << k)))
            L.add("add/cancel-into-denormal", enc(sa, e, x), enc(sb, e, (x ^ (r64() >> (e + 1))) | TOP))
            if e > 1:
                L.add("add/cancel-into-denormal", enc(sa, e, TOP | (r64() >> 60)), enc(sb, e - 1, ALL - (r64() >> 60)))

    # ---- add, the general path
    for k in range(24):
        for sa, sb in SIGNS:
            L.both("add/denormal-denormal", enc(sa, 0, r64() >> (1 + k % 40)), enc(sb, 0, r64() >> (1 + (7 * k) % 50)))
    for sa, sb in SIGNS:                       # a carry from exponent 0 into exponent 1
        L.both("add/denormal-carry", enc(sa, 0, TOP - 1), enc(sb, 0, 1))
        L.both("add/denormal-carry", enc(sa, 0, TOP - 1), enc(sb, 0, TOP - 1))
        L.both("add/denormal-carry", enc(sa, 0, (TOP >> 1) | (r64() >> 2)), enc(sb, 0, (TOP >> 1) | (r64() >> 2)))
    for e in range(1, 71):
        for sa, sb in SIGNS:
            L.both("add/denormal-normal", enc(sa, 0, r64() >> (1 + e % 9)), enc(sb, e, r64() | TOP))
            L.both("add/smallest-denormal", enc(sa, 0, 1), enc(sb, e, r64() | TOP))
    for sa, sb in SIGNS:
        for k in range(6):
            pseudo = enc(sa, 0, TOP | (r64() >> (1 + 9 * k)))
            L.both("add/pseudo-denormal", pseudo, enc(sb, 0, r64() >> (1 + 5 * k)))
            L.both("add/pseudo-denormal", pseudo, enc(sb, 1 + 13 * k, r64() | TOP))
            L.both("add/pseudo-denormal", pseudo, enc(sb, 0, TOP | (r64() >> (1 + 3 * k))))
            L.both("add/pseudo-denormal-zero", pseudo, enc(sb, 0, 0))
        L.both("add/zeros", enc(sa, 0, 0), enc(sb, 0, 0))
    for x in _representatives(rng):
        for sb in (0, 1):
            L.both("add/smallest-denormal", enc(sb, 0, 1), x)
        if classify(x) in FINITE:              # exact cancellation: +0
            L.both("add/exact-cancel", x, (x[0], x[1] ^ 0x8000))

    # ---- mul
    for raw in list(MUL_LOW) + list(MUL_HIGH):
        # two normals whose product has this raw exponent (or one more, when
        # the significands' product reaches 2^127)
        for k in range(10):
            ea = int(rng.integers(max(1, raw + BIAS - EMAX), min(EMAX, raw + BIAS - 1) + 1))
            eb = raw + BIAS - ea
            ma, mb = r64() | TOP, r64() | TOP
            if (ma * mb) >> 127:
                eb -= 1
            if k >= 6:                          # a short product: exact unless denormalised
                ma, mb = TOP | (r64() >> 40 << 39), TOP | (r64() >> 40 << 39)
                eb = raw + BIAS - ea - ((ma * mb) >> 127)
            if not 1 <= eb <= EMAX:
                continue
            L.add("mul/exponent", enc(k & 1, ea, ma), enc((k >> 1) & 1, eb, mb))
    for k in range(1, 65):                      # around half of the smallest denormal
        ea = 1 + 97 * k
        eb = -63 + BIAS - ea
        L.add("mul/half-smallest", enc(k & 1, ea, TOP), enc(0, eb, TOP))               # exactly half: a tie to zero
        L.add("mul/half-smallest", enc(k & 1, ea, TOP), enc(0, eb, TOP | k))           # just over: the smallest denormal
        L.add("mul/half-smallest", enc(k & 1, ea, ALL), enc(0, eb - 2, ALL - k))       # just under: zero
        L.add("mul/largest-denormal", enc(k & 1, ea, ALL), enc(0, BIAS - 1 - ea, ALL - k))  # rounds up to the smallest normal
        L.add("mul/largest-denormal", enc(k & 1, ea, ALL - (k << 20)), enc(0, BIAS - ea, TOP))
    for sa, sb in SIGNS:
        for e in (BIAS, 1, EMAX, BIAS + 8191, BIAS - 8191):
            L.add("mul/all-ones", enc(sa, e, ALL), enc(sb, min(EMAX, max(1, 2 * BIAS - e)), ALL))
    # exact ties: (2^63 + x)(2^63 + y) = 2^126 + (x + y) 2^63 + xy with
    # xy = 2^62 (mod 2^63); both parities of the kept significand
    for x in range(1, 64, 2):
        L.both("mul/tie", enc(0, BIAS + x, TOP + x), enc(x & 2 and 1, BIAS - x, TOP + QUIET))
    for j in range(1, 31):
        L.both("mul/tie", enc(0, BIAS - j, TOP + (1 << j)), enc(1, BIAS + 2 * j, TOP + (1 << (62 - j))))
        L.both("mul/tie", enc(1, BIAS + j, TOP + 3 * (1 << j)), enc(1, BIAS, TOP + (1 << (62 - j))))
    # rounding carries out: (2^64 - 2y)(2^63 + y) = 2^127 - 2y^2
    for y in range(1, 33):
        L.both("mul/round-carry", enc(y & 1, BIAS + 5 * y, ALL + 1 - 2 * y), enc(0, BIAS - 3 * y, TOP + y))
        L.add("mul/round-carry", enc(0, EMAX - y, ALL + 1 - 2 * y), enc(y & 1, BIAS + y, TOP + y))       # into overflow
        L.add("mul/round-carry", enc(0, y, ALL + 1 - 2 * y), enc(y & 1, BIAS - y, TOP + y))              # largest denormal up
    for k in range(64):                         # exact: at most 32 significant bits each
        ma, mb = (r64() >> 32 | (1 << 31)) << 32, (r64() >> 32 | (1 << 31)) << 32
        L.add("mul/exact", enc(k & 1, BIAS - 100 + 3 * k, ma), enc((k >> 1) & 1, BIAS + 50 - 2 * k, mb))
    for k in range(64):
        den = enc(k & 1, 0, r64() >> (1 + k % 60))
        L.both("mul/denormal-normal", den, enc((k >> 1) & 1, BIAS + k % 64 + k // 8, r64() | TOP))
        L.both("mul/denormal-normal", den, enc((k >> 1) & 1, EMAX - k % 5, r64() | TOP))
        L.both("mul/denormal-denormal", den, enc((k >> 1) & 1, 0, r64() >> (1 + k % 7)))
        L.both("mul/pseudo-denormal", enc(k & 1, 0, r64() | TOP), enc((k >> 1) & 1, BIAS + k % 3, r64() | TOP))

    # ---- specials, for all four ops: every representative against every other
    reps = _representatives(rng)
    for i, x in enumerate(reps):
        for y in reps[i:]:
            cx, cy = classify(x), classify(y)
            if cx in FINITE and cy in FINITE:
                continue
            L.both("special/%s,%s" % tuple(sorted((cx, cy))), x, y)
    qa, qb = TOP | QUIET | 0x77, TOP | QUIET | 0x78
    sn, sm = TOP | 0x77, TOP | 0x78
    for sa, sb in SIGNS:
        L.both("special/nan-quiet-payloads", enc(sa, 0x7FFF, qa), enc(sb, 0x7FFF, qb))
        L.both("special/nan-signalling-payloads", enc(sa, 0x7FFF, sn), enc(sb, 0x7FFF, sm))
        L.both("special/nan-quiet-signalling", enc(sa, 0x7FFF, qa), enc(sb, 0x7FFF, sm))   # larger payload signalling
        L.both("special/nan-quiet-signalling", enc(sa, 0x7FFF, qb), enc(sb, 0x7FFF, sn))
        L.both("special/nan-quiet-signalling", enc(sa, 0x7FFF, qa), enc(sb, 0x7FFF, sn | QUIET >> 1))
    for s in (0, 1):                             # equal significands, different signs
        L.both("special/nan-equal-significands", enc(s, 0x7FFF, qa), enc(1 - s, 0x7FFF, qa))
        L.both("special/nan-equal-significands", enc(s, 0x7FFF, sn), enc(1 - s, 0x7FFF, sn))
        L.both("special/nan-equal-significands", enc(s, 0x7FFF, sn), enc(1 - s, 0x7FFF, sn | QUIET))
    for sa, sb in SIGNS:
        L.both("special/inf-inf", enc(sa, 0x7FFF, TOP), enc(sb, 0x7FFF, TOP))
        L.both("special/zero-inf", enc(sa, 0, 0), enc(sb, 0x7FFF, TOP))
        L.both("special/inf-denormal", enc(sa, 0x7FFF, TOP), enc(sb, 0, 1))
        L.both("special/inf-denormal", enc(sa, 0x7FFF, TOP), enc(sb, 0, r64() >> 3))
        L.both("special/inf-denormal", enc(sa, 0x7FFF, TOP), enc(sb, 0, TOP | r64()))

    # ---- compare, for min and max
    for sa, sb in SIGNS:
        L.both("compare/zeros", enc(sa, 0, 0), enc(sb, 0, 0))
        for k in range(4):
            m = TOP | (r64() >> (1 + 16 * k))
            L.both("compare/pseudo-denormal-same-value", enc(sa, 0, m), enc(sb, 1, m))
            L.both("compare/pseudo-denormal-neighbours", enc(sa, 0, m), enc(sb, 1, m + 1))
            L.both("compare/pseudo-denormal-neighbours", enc(sa, 0, m), enc(sb, 0, TOP - 1))
            L.both("compare/denormal-zero", enc(sa, 0, r64() >> (1 + 15 * k)), enc(sb, 0, 0))
            L.both("compare/largest-finite-inf", enc(sa, EMAX, ALL - k), enc(sb, 0x7FFF, TOP))
            L.both("compare/neighbours", enc(sa, BIAS + k, m), enc(sb, BIAS + k, m ^ 1))
            L.both("compare/neighbours", enc(sa, BIAS + k, TOP), enc(sb, BIAS + k - 1, ALL))
    for x in _representatives(rng):
        if x[1] & 0x8000 == 0 and classify(x) in FINITE + ("inf",):
            L.both("compare/opposite-signs", x, (x[0], x[1] ^ 0x8000))
            L.both("compare/equal", x, x)

    assert len(L.a) <= MAX_PAIRS
    return L


_CACHE = {}


def pairs(drop=()):
    """(a, b, groups): the whole list; a and b np.longdouble, read-only, and
    groups[i] the name of pair i's group.  drop: group name prefixes to leave
    out (for checking that the census test notices)."""
    key = tuple(drop)
    if key not in _CACHE:
        L = _build()
        keep = [i for i, g in enumerate(L.groups) if not any(g.startswith(d) for d in drop)]
        a, b = to_slots([L.a[i] for i in keep]), to_slots([L.b[i] for i in keep])
        a.flags.writeable = b.flags.writeable = False
        _CACHE[key] = (a, b, tuple(L.groups[i] for i in keep))
    return _CACHE[key]


def select(groups, *prefixes):
    """Indices of the pairs whose group starts with one of the prefixes."""
    return np.array([i for i, g in enumerate(groups) if g.startswith(prefixes)], dtype=np.int64)


def shortfalls(groups, cen):
    """What the list must hold, as conditions: the census classes and groups
    that are below their minimum (none, for the list as it stands)."""
    c = counts(cen)
    need = {"add:d=%d:%s%s" % (d, x, y): 5 for d in range(DMAX + 1) for x in "+-" for y in "+-"}
    for lab in ("add:tie:even", "add:tie:odd", "add:round-carry", "add:overflow", "add:cancel-into-denormal",
                "mul:tie:even", "mul:tie:odd", "mul:round-carry"):
        need[lab] = 8
    for raw in list(MUL_LOW) + list(MUL_HIGH):
        need["mul:e=%d" % raw] = 8
    for op in ("add", "mul"):
        for res in ("normal", "denormal", "zero", "inf", "nan"):
            need["%s:res=%s" % (op, res)] = 1
    for cmp in ("lt", "gt", "neither"):
        need["cmp:" + cmp] = 1
    short = ["%s: %d < %d" % (lab, c.get(lab, 0), k) for lab, k in sorted(need.items()) if c.get(lab, 0) < k]
    have = set(groups)
    for base in REQUIRED_GROUPS:
        for order in ("/ab", "/ba"):
            if base + order not in have:
                short.append("group %s%s is empty" % (base, order))
    for g in sorted(have):
        if g.startswith(("special/", "compare/")) and g[:-3] not in REQUIRED_GROUPS:
            short.append("group %s is not in REQUIRED_GROUPS" % g)
    return short


_CLASSES = ("zero", "denormal", "pseudo-denormal", "normal", "inf", "qnan", "snan", "pseudo-inf", "pseudo-nan",
            "unnormal")
REQUIRED_GROUPS = tuple(
    ["special/%s,%s" % (x, y) for i, x in enumerate(sorted(_CLASSES)) for y in sorted(_CLASSES)[i:]
     if not (x in FINITE and y in FINITE)]
    + ["special/" + g for g in ("nan-quiet-payloads", "nan-signalling-payloads", "nan-quiet-signalling",
                                "nan-equal-significands", "inf-inf", "zero-inf", "inf-denormal")]
    + ["compare/" + g for g in ("zeros", "pseudo-denormal-same-value", "pseudo-denormal-neighbours",
                                "denormal-zero", "largest-finite-inf", "neighbours", "opposite-signs", "equal")])


def broad(cen, idx=None):
    """counts() with the per-distance and per-exponent labels folded into one
    line each: what a route ran, short enough to print."""
    out = Counter()
    for lab, k in counts(cen, idx).items():
        if lab.startswith(("cls:", "cmp:")) or ":general:" in lab:
            continue
        key = "add:normal+normal" if lab.startswith("add:d=") else \
            "mul:denormal-range" if lab.startswith("mul:e=") and int(lab[6:]) < 1000 else \
            "mul:overflow-boundary" if lab.startswith("mul:e=") else lab
        out[key] += k
    return dict(sorted(out.items()))


# ------------------------------------------------------------------ the chains
def host_op(op, a, b):
    """a op b on the host's x87, as the reference folds (reduce-op.c: a + b,
    a * b, a < b ? a : b, a > b ? a : b)."""
    with np.errstate(all="ignore"):
        if op == "sum":
            return a + b
        if op == "prod":
            return a * b
        return np.where(a < b, a, b) if op == "min" else np.where(a > b, a, b)


def third(op, a, b):
    """The third operand of a three-input fold, from the host's r = a op b,
    by index mod 4: -r (exact cancellation for sum); r's exponent less 64
    with significand 2^63 (a tie for sum); r's exponent less 65 with
    significand 2^63 | 1 (sticky from bit 0); and for prod an exponent that
    puts r * c on the denormal and overflow boundaries in turn, for the other
    ops r's neighbour with the opposite sign.  Exponents are kept in 1..0x7FFE,
    going above r where there is no room below."""
    rng = np.random.default_rng(0xC4A1)
    r = from_slots(host_op(op, a, b))
    flips = rng.integers(0, 2, len(r))
    targets = list(range(-65, 3)) + list(MUL_HIGH)
    out = []
    for i, (sig, se) in enumerate(r):
        e, neg = se & 0x7FFF, se >> 15
        k = i % 4
        if k == 0:
            c = (sig, se ^ 0x8000)
        elif k in (1, 2):
            d = 63 + k
            ec = e - d if e - d >= 1 else min(EMAX, e + d)
            c = enc(int(flips[i]) ^ neg, ec, TOP if k == 1 else TOP | 1)
        elif op == "prod":
            raw = targets[(i // 4) % len(targets)]
            c = enc(int(flips[i]), min(EMAX, max(1, raw + BIAS - max(e, 1))), TOP | (sig >> 1) | 1)
        else:
            c = enc(1 - neg, min(EMAX, max(1, e)), (sig ^ 1) | TOP)
        out.append(c)
    return to_slots(out)


# ------------------------------------------------------------- complex product
def annex_g_operands(t):
    """Every pair of the 64 complex numbers whose parts are drawn from
    {0, -0, 1, -2, +-inf, NaN, 3.5}: the operands on which Annex G's recovery
    of infinities (__muldc3 / __mulsc3) decides the product."""
    ft, ct = (np.float64, np.complex128) if t == "complexd" else (np.float32, np.complex64)
    parts = np.array([0.0, -0.0, 1.0, -2.0, np.inf, -np.inf, np.nan, 3.5], dtype=ft)
    zs = np.array([complex(x, y) for x in parts for y in parts], dtype=ct)
    return np.repeat(zs, len(zs)), np.tile(zs, len(zs))


def assert_annex_g(got, want, what):
    """NaN exactly where the oracle has NaN, identical bytes everywhere else."""
    for comp in ("real", "imag"):
        g, w = getattr(got, comp), getattr(want, comp)
        bad = np.flatnonzero(np.isnan(g) != np.isnan(w))
        assert bad.size == 0, (what, comp, "NaN placement differs, first at", bad[:4])
        m = ~np.isnan(w)
        gb = np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1)
        wb = np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1)
        bad = np.flatnonzero(m & (gb != wb).any(axis=1))
        assert bad.size == 0, (what, comp, "bytes differ, first at", bad[:4])
