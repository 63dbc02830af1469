"""TEST INFRASTRUCTURE: the DC tracker of csrc/dc_block.hpp restated in numpy.

A component c is the float32 the load stage makes of a sample (balance_model.convert).  q(c) = rint(c' 2^32) as int64, c' = c
clamped to +-64, a NaN counting 0.  The stream is cut into blocks of B = 2^log2 samples aligned to the stream position;
S_k = the int64 sum of q over block k per arm; m_k = float32(float64(S_k) / (B 2^32)); a sample of block k >= 1 becomes
(i - m_{k-1}.i, q - m_{k-1}.q) in float32, block 0 uses the seed; a NaN component leaves with its quiet bit set."""
import numpy as np

MIN_LOG2, MAX_LOG2, DEFAULT_LOG2 = 12, 24, 20


def quant(c):
    """c: float32 array of any bit patterns -> int64"""
    c = np.ascontiguousarray(c, np.float32)
    nan = np.isnan(c)
    with np.errstate(all="ignore"):
        cc = np.clip(np.where(nan, np.float32(0), c), np.float32(-64), np.float32(64))
        q = np.rint(cc.astype(np.float64) * 2.0**32)
    return q.astype(np.int64)


def mean_of(total, count):
    """float32(float64(total) / (count 2^32)); total an int (exact in int64)"""
    return np.float32(np.float64(np.int64(total)) / (float(count) * 2.0**32))


def head_mean(x, n):
    """what irdm_dc_mean_host gives for the n leading samples of the interleaved float32 x"""
    q = quant(x[:2 * n])
    return mean_of(int(q[0::2].sum()), n), mean_of(int(q[1::2].sum()), n)


def subtract(x, m_i, m_q):
    """x: float32 [2 n] interleaved -> x - (m_i, m_q) in float32, NaN components quieted in place"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    with np.errstate(all="ignore"):
        y[0::2] = x[0::2] - np.float32(m_i)
        y[1::2] = x[1::2] - np.float32(m_q)
    nan = np.isnan(x)
    y.view(np.uint32)[nan] = x.view(np.uint32)[nan] | np.uint32(0x00400000)
    return y


def run(x, log2, seed=(0.0, 0.0), first=0, sums=(0, 0)):
    """x: float32 [2 n] interleaved, the samples at stream positions first .. first + n; `sums`: the sums of the block `first`
    lies in as far as the stream has been seen (ignored on a block edge); seed: the mean that block is corrected by.
    Returns (y, state, means): the corrected samples, (sum_i, sum_q, mean_i, mean_q) as irdm_dc_block_device leaves them in
    state_io, and [(k, m_i, m_q)] for every block closed."""
    x = np.ascontiguousarray(x, np.float32)
    n, B = len(x) // 2, 1 << log2
    y = np.empty_like(x)
    q = quant(x)
    m = (np.float32(seed[0]), np.float32(seed[1]))
    s = [int(sums[0]), int(sums[1])] if first % B else [0, 0]
    means = []
    at = 0
    while at < n:
        pos = first + at
        k = pos >> log2
        run_n = min(n - at, (k + 1) * B - pos)
        y[2 * at:2 * (at + run_n)] = subtract(x[2 * at:2 * (at + run_n)], *m)
        s[0] += int(q[2 * at:2 * (at + run_n):2].sum())
        s[1] += int(q[2 * at + 1:2 * (at + run_n):2].sum())
        at += run_n
        if (first + at) % B == 0:
            m = (mean_of(s[0], B), mean_of(s[1], B))
            means.append((k, m[0], m[1]))
            s = [0, 0]
    return y, (s[0], s[1], m[0], m[1]), means


def dc_model(x, log2=DEFAULT_LOG2, seed=(0.0, 0.0)):
    """a whole stream from position 0: (y, figures) with the figures irdm_dc_stats reports"""
    y, state, means = run(x, log2, seed)
    fig = dict(n_samples=len(x) // 2, n_blocks=len(means), block_log2=log2, seed=(np.float32(seed[0]), np.float32(seed[1])),
               first=(0.0, 0.0), last=(0.0, 0.0), min=(0.0, 0.0), max=(0.0, 0.0))
    if means:
        mi, mq = np.array([m[1] for m in means], np.float32), np.array([m[2] for m in means], np.float32)
        fig.update(first=(mi[0], mq[0]), last=(mi[-1], mq[-1]), min=(mi.min(), mq.min()), max=(mi.max(), mq.max()))
    return y, fig
