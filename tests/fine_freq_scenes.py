"""TEST INFRASTRUCTURE: the scenes the carrier frequency tests share (tests/test_fine_freq_model.py, tests/test_gpu_fine_freq*.py)
and their truth: the frequency each burst was generated at, at the middle of the frame the downmixer cut from it."""
import functools

import numpy as np

import orc
import siggen

CENTER = 1622000000.0
START_NS = 1700000000 * 10**9
OUT_RATE = 250000.0
DRIFT = 390.0          # Hz/s: about the largest Doppler rate of an Iridium pass at L band


@functools.lru_cache(maxsize=None)
def standard(fs, seed, amp):
    """(iq, truth) of siggen.standard_scene(fs, fs, 16, seed, amp=amp): one second, 16 bursts at constant frequencies"""
    iq, truth = siggen.standard_scene(fs, fs, 16, seed, amp=amp)
    for t in truth:
        t["rate"] = 0.0
    iq.setflags(write=False)
    return iq, truth


@functools.lru_cache(maxsize=None)
def drifting(seed, fs=2_000_000, n_bursts=12):
    """(iq, truth): n_bursts bursts at fs, each with a linear drift of +-DRIFT Hz/s (the sign alternates); freq_hz is the
    frequency at the burst's first sample"""
    rng = np.random.default_rng(seed + 2000)
    n = fs
    iq = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)).astype(np.complex64)
    iq *= np.float32(0.002)
    first = 520 * 2048
    starts = np.sort(rng.integers(0, n - first - fs // 20, size=n_bursts)) + first
    half_ch = int((fs / 2 - 60e3) // (1e6 / 24.0))
    truth = []
    for i, s in enumerate(starts):
        payload = rng.integers(0, 4, size=int(rng.integers(119, 180))).tolist()
        ch = int(rng.integers(-half_ch, half_ch + 1)) or 1
        f0, rate = siggen.channel_freq(ch), DRIFT * (1 if i % 2 == 0 else -1)
        sig = siggen.make_burst(fs, siggen.frame_quadrants(payload), 0.0, 0.0, 0.05).astype(np.complex128)
        t = np.arange(len(sig), dtype=np.float64) / fs
        sig = sig * np.exp(1j * (2 * np.pi * (f0 * t + 0.5 * rate * t * t) + rng.uniform(0, 2 * np.pi)))
        e = min(n, int(s) + len(sig))
        iq[int(s):e] += sig[:e - int(s)].astype(np.complex64)
        truth.append(dict(start=int(s), freq_hz=f0, rate=rate, n=len(sig)))
    iq.setflags(write=False)
    return iq, truth


def truth_of(truth, fs, timestamp_ns, num_samples, center_frequency):
    """the absolute frequency [Hz] the scene has at the middle of a frame: the burst that starts nearest in front of the
    frame's time on the channel of center_frequency (any estimate of it: channels are 41.7 kHz apart)"""
    t_mid = (timestamp_ns - START_NS) * 1e-9 + 0.5 * num_samples / OUT_RATE
    best = None
    for b in truth:
        if abs(CENTER + b["freq_hz"] - center_frequency) > 2000.0:
            continue
        dt = t_mid - b["start"] / fs
        if -0.002 <= dt <= b["n"] / fs + 0.002 and (best is None or dt < best[0]):
            best = (dt, b)
    assert best is not None, (t_mid, center_frequency)
    dt, b = best
    return CENTER + b["freq_hz"] + b["rate"] * dt


@functools.lru_cache(maxsize=None)
def oracle(kind, *key):
    """the CPU oracle's run over a scene: kind "standard" (fs, seed, amp) or "drifting" (seed)"""
    iq, truth = standard(*key) if kind == "standard" else drifting(*key)
    fs = key[0] if kind == "standard" else 2_000_000
    return orc.run_stream(iq, fs, start_time_ns=START_NS), truth, fs


def oracle_frames(kind, *key):
    """[(samples complex64, downmixer's frequency, PLL's frequency, truth)] of the frames whose unique word passed"""
    r, truth, fs = oracle(kind, *key)
    frames = {f.id: f for f in r.frames if f.drop_reason == 0}
    out = []
    for d in r.demods:
        f = frames[d.id]
        x = np.array(f.samples[:2 * f.num_samples], np.float32).view(np.complex64)
        out.append((x, f.center_frequency, d.center_frequency, truth_of(truth, fs, f.timestamp, f.num_samples, f.center_frequency)))
    return out
