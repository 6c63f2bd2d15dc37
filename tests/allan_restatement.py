"""Reference-shaped numpy restatement of the Allan variance (src/allanvariance/allan_gyr.cc of the reference), the yardstick
of tests/test_allan*.py: sequential running sums, the factor list with the float truncations of getLogSpace, and the
variance per factor."""
import math

import numpy as np


def factors(n, num_clusters=10000):
    """initStrides + getLogSpace (:141-196)."""
    mode = int(n) // 2
    max_stride, shft = 1, 0
    while mode:
        mode >>= 1
        max_stride = 1 << shft
        shft += 1
    b = float(np.float32(math.log10(max_stride)))                     # getLogSpace(float a, float b)
    start = math.pow(10, 0.0)
    end = math.pow(10, b)
    progression = math.pow(end / start, float(np.float32(1) / np.float32(num_clusters - 1)))
    ls = [start]
    for _ in range(1, num_clusters):
        ls.append(ls[-1] * progression)
    out = []
    prev = None
    for v in ls:
        c = math.ceil(v)
        if c != prev:
            out.append(c)
        prev = c
    return np.array(out, dtype=np.int64)


def host_values(t_s):
    """getAvgDt (:205-214): sequential sum of consecutive differences; freq = 1 / avgDt, period = avgDt."""
    t = np.asarray(t_s, dtype=np.float64)
    s = 0.0
    for d in np.diff(t).tolist():
        s += d
    avg = s / (len(t) - 1)
    return 1.0 / avg, avg


def seq_mean(w):
    """getAvgValue: sequential sum / n."""
    s = 0.0
    for x in np.asarray(w, dtype=np.float64).tolist():
        s += x
    return s / len(w)


def thetas(w, freq):
    """calcThetas (:130-139): sequential running sum, every prefix divided by freq."""
    return np.cumsum(np.asarray(w, dtype=np.float64)) / freq


def variance(theta, period, fac):
    """calcVariance (:104-125); NaN where n - 2m <= 0."""
    n = len(theta)
    out = np.empty(len(fac))
    for i, m in enumerate(np.asarray(fac).tolist()):
        if n - 2 * m <= 0:
            out[i] = np.nan
            continue
        d = theta[2 * m:] - 2 * theta[m:n - m] + theta[:n - 2 * m]
        out[i] = np.dot(d, d) / (2 * (period * m) * (period * m) * (n - 2 * m))
    return out


def rounding_bound(theta, fac):
    """8 eps max|theta| / rms(second difference) at the smallest factor: how far a reordered sum may move sigma2."""
    m = int(fac[0])
    d = theta[2 * m:] - 2 * theta[m:len(theta) - m] + theta[:len(theta) - 2 * m]
    return 8 * np.finfo(np.float64).eps * np.abs(theta).max() / np.sqrt(np.mean(d * d))


def model_sigma2(p, tau):
    tau = np.asarray(tau, dtype=np.float64)
    return p[0] ** 2 / tau ** 2 + p[1] ** 2 / tau + p[2] ** 2 + p[3] ** 2 * tau + p[4] ** 2 * tau ** 2
