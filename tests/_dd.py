"""Double-word arithmetic on NumPy ``longdouble`` arrays (TEST INFRASTRUCTURE: the working precision of tests/_xref.py).  A number is the
unevaluated sum hi + lo of two longdoubles, |lo| <= ulp(hi) / 2: about 128 bits of significand on x86-64, so that a row of the
extended-precision reference ROUNDED to longdouble is the correctly rounded truth even where the reference's formulas subtract nearly
equal numbers (np.diff of kappa, theta - theta_ref from a standstill, d'' next to a stop).  The error-free transformations are Knuth's
two-sum and Dekker's product with a 32 / 32 split of the 64-bit significand; +, -, *, /, sqrt after Hida, Li and Bailey's double-double
algorithms; sin, cos, atan by argument reduction, Taylor series and one Newton step.  NumPy only."""
import numpy as np

LD = np.longdouble
_SPLIT = LD(2 ** 32 + 1)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class DD:
    __slots__ = ("hi", "lo")
    __array_ufunc__ = None   # (ndarray op DD is DD's business)

    def __init__(self, hi, lo=None):
        self.hi = np.asarray(hi, dtype=LD)
        self.lo = np.zeros_like(self.hi) if lo is None else np.asarray(lo, dtype=LD)

    @staticmethod
    def of(x):
        return x if isinstance(x, DD) else DD(x)

    # ---- shape ----
    @property
    def shape(self):
        return np.broadcast(self.hi, self.lo).shape

    def __getitem__(self, k):
        return DD(self.hi[k], self.lo[k])

    def __setitem__(self, k, v):
        v = DD.of(v)
        self.hi[k], self.lo[k] = v.hi, v.lo

    def copy(self):
        return DD(self.hi.copy(), self.lo.copy())

    def ld(self):
        """rounded to longdouble"""
        return np.asarray(self.hi + self.lo, dtype=LD)

    # ---- arithmetic ----
    def __neg__(self):
        return DD(-self.hi, -self.lo)

    def __abs__(self):
        neg = (self.hi < 0) | ((self.hi == 0) & (self.lo < 0))
        return DD(np.where(neg, -self.hi, self.hi), np.where(neg, -self.lo, self.lo))

    def __add__(self, o):
        o = DD.of(o)
        s1, s2 = _two_sum(self.hi, o.hi)
        t1, t2 = _two_sum(self.lo, o.lo)
        s1, s2 = _quick_two_sum(s1, s2 + t1)
        return DD(*_quick_two_sum(s1, s2 + t2))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-DD.of(o))

    def __rsub__(self, o):
        return DD.of(o) + (-self)

    def __mul__(self, o):
        o = DD.of(o)
        p, e = _two_prod(self.hi, o.hi)
        return DD(*_quick_two_sum(p, e + (self.hi * o.lo + self.lo * o.hi)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = DD.of(o)
        q1 = self.hi / o.hi
        r = self - o * DD(q1)
        q2 = r.hi / o.hi
        r = r - o * DD(q2)
        q3 = r.hi / o.hi
        return DD(*_quick_two_sum(q1, q2)) + DD(q3)

    def __rtruediv__(self, o):
        return DD.of(o) / self

    def __pow__(self, k):
        assert k == 2
        return self * self

    def scaled(self, power_of_two):
        """times an exact power of two"""
        f = LD(power_of_two)
        return DD(self.hi * f, self.lo * f)

    # ---- comparisons (arrays of bool) ----
    def _sign_of_difference(self, o):
        d = self - DD.of(o)
        return np.where(d.hi != 0, d.hi, d.lo)

    def __lt__(self, o):
        return self._sign_of_difference(o) < 0

    def __le__(self, o):
        return self._sign_of_difference(o) <= 0

    def __gt__(self, o):
        return self._sign_of_difference(o) > 0

    def __ge__(self, o):
        return self._sign_of_difference(o) >= 0


def where(cond, a, b):
    a, b = DD.of(a), DD.of(b)
    return DD(np.where(cond, a.hi, b.hi), np.where(cond, a.lo, b.lo))


def zeros(shape):
    return DD(np.zeros(shape, dtype=LD))


def broadcast_to(a, shape):
    a = DD.of(a)
    return DD(np.broadcast_to(a.hi, shape).copy(), np.broadcast_to(a.lo, shape).copy())


def stack(items, axis=0):
    return DD(np.stack([DD.of(x).hi for x in items], axis=axis), np.stack([DD.of(x).lo for x in items], axis=axis))


def sqrt(a):
    a = DD.of(a)
    x = np.sqrt(a.hi)
    safe = np.where(x == 0, LD(1), x)
    corr = (a - DD(x) * DD(x)).hi / (2 * safe)
    return DD(x) + DD(np.where(x == 0, LD(0), corr))


def total(a, axis_len, take):
    """plain sum, in order, of take(i) for i < axis_len"""
    out = take(0)
    for i in range(1, axis_len):
        out = out + take(i)
    return out


# pi / 2 = hi + lo
PIO2 = DD(LD("1.570796326794896619231322"), LD("-2.508278806334166011778664e-20"))


def sincos(a):
    """(sin a, cos a): a = k pi/2 + r, Taylor series of r / 32, five angle doublings"""
    a = DD.of(a)
    k = np.rint(a.hi / PIO2.hi)
    r = a - DD(k) * PIO2
    x = r.scaled(2.0 ** -5)
    x2 = x * x
    s, c = x, DD(np.ones_like(x.hi))
    ts, tc = x, DD(np.ones_like(x.hi))
    for j in range(1, 13):
        tc = -(tc * x2) / DD(LD((2 * j - 1) * (2 * j)))
        ts = -(ts * x2) / DD(LD((2 * j) * (2 * j + 1)))
        c, s = c + tc, s + ts
    for _ in range(5):
        s, c = (s * c).scaled(2.0), c * c - s * s
    q = np.mod(k, 4)
    sin = where(q == 0, s, where(q == 1, c, where(q == 2, -s, -c)))
    cos = where(q == 0, c, where(q == 1, -s, where(q == 2, -c, s)))
    return sin, cos


def atan(x):
    """arctan x: longdouble's, then one Newton step on tan t = x"""
    x = DD.of(x)
    t0 = DD(np.arctan(x.hi))
    s, c = sincos(t0)
    return t0 + (x * c - s) * c


def mod(a, m):
    """a mod m with the sign of m > 0 (Python's and NumPy's %)"""
    a, m = DD.of(a), DD.of(m)
    q = np.floor((a / m).hi)
    r = a - DD(q) * m
    r = where(r < 0, r + m, r)
    return where(r >= m, r - m, r)
