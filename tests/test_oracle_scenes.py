"""CPU: the edge-case scenes really exercise what they claim (the oracle's view), so the GPU parity tests on the
same scenes (test_gpu_scenes.py) cover those branches of the reference's state machine."""
import hashlib

import numpy as np
import pytest

import orc
import scenes


def test_squelch_scene_dumps_resets_and_recovers():
    fs, iq = scenes.squelch()
    r = orc.run_stream(iq, fs)
    early = [b for b in r.bursts if b.start < 530 * 2048 + 1_000_000]
    late = [b for b in r.bursts if b.start >= 530 * 2048 + 2_000_000]
    assert len(early) >= 30                                   # the dumped wave
    assert max(b.stop - b.start for b in early) < 20_000      # squelched long before a normal burst would end
    assert len(late) == 6 and len(r.demods) == 6              # decoded again after re-priming


def test_too_long_scene_forces_burst_ends():
    fs, iq = scenes.too_long()
    r = orc.run_stream(iq, fs)
    max_len = int(0.09 * fs)
    assert sum(1 for b in r.bursts if b.stop - b.start > max_len) >= 2
    assert len(r.demods) >= 3


def test_dc_scene_never_centres_a_burst_on_the_notch():
    fs, iq = scenes.dc_and_edges()
    r = orc.run_stream(iq, fs)
    n = 2048
    assert r.bursts and all(abs(b.center_bin - n // 2) > 3 for b in r.bursts)
    assert all(40 // 2 <= b.center_bin < n - 40 // 2 for b in r.bursts)


def test_many_active_scene_exceeds_the_sparse_scan_slots():
    fs, iq = scenes.many_active_10m()
    r = orc.run_stream(iq, fs)
    ev = sorted([(b.start, 1) for b in r.bursts] + [(b.stop, -1) for b in r.bursts])
    cur = peak = 0
    for _, d in ev:
        cur += d
        peak = max(peak, cur)
    assert peak > 64 and len(r.demods) >= 70


# sha256 of each scene's samples at its default rate, computed before the scenes took a rate: scenes._Layout must leave the
# default scenes the same bytes (every test on them keeps checking what it checked)
DEFAULT_DIGESTS = {
    "squelch": (2_000_000, 5373952, "01a0414a9c08cf83dcd4205135737ea5606143f568eb0a65bd164e18e2f8c2dc"),
    "too_long": (2_000_000, 2981888, "a555ed4c2ee28dc647848e6bdbca4ce3fb86ebb8982a56135c94f1bc8e81a38f"),
    "dc_and_edges": (2_000_000, 2588672, "1035043d69bcb4ae8119ee8601292d31fca262236d3a8721835e8b5d1274714b"),
    "strong_simultaneous": (2_000_000, 2588672, "2fd6986362d4f52670f2c910d9455cf7180ceff739089980766c32b8434cf01b"),
    "many_active_10m": (10_000_000, 7471104, "a1284134e763657a8c61fc3bdb4fafd57f4686c077598de8dde216617c7751b8"),
    "frame_lengths": (2_000_000, 3768320, "d3a5df73e4f2b1ee3e40d7fa04dd4dce574d59f3679d2e5ae8eadcce6dc61d5f"),
    "junk": (2_000_000, 3768320, "e14a0e103cb28d6c054b305bbc7ca5aa8debf50df4c3069d1d6e42a6bf8019ae"),
    "cfo_spread": (2_000_000, 3768320, "d82f6eb67c74b4c599faf4e2eaa515ab2b72104156f0f05d6e40d862edf48a66"),
    "frame_lengths_simplex": (2_000_000, 3768320, "c5da80aa5e56d4d954b7077cc6dbffb2d34ecf8ae0cdaa42e8815559995a4738"),
}


@pytest.mark.parametrize("name", sorted(DEFAULT_DIGESTS))
def test_default_scenes_are_the_bytes_they_were(name):
    fs, iq = scenes.frame_lengths(simplex=True) if name == "frame_lengths_simplex" else scenes.ALL[name]()
    assert (fs, len(iq), hashlib.sha256(iq.tobytes()).hexdigest()) == DEFAULT_DIGESTS[name]


def _peak_active(bursts):
    ev = sorted([(b.start, 1) for b in bursts] + [(b.stop, -1) for b in bursts])
    cur = peak = 0
    for _, d in ev:
        cur += d
        peak = max(peak, cur)
    return peak


@pytest.mark.parametrize("name,fs,min_bursts,min_demods", [
    ("too_long", 16_000_000, 8, 3), ("too_long", 12_500_000, 8, 3),
    ("strong_simultaneous", 16_000_000, 8, 6), ("strong_simultaneous", 12_500_000, 8, 6), ("strong_simultaneous", 8_000_000, 8, 6),
    ("dc_and_edges", 20_000_000, 4, 4), ("many_active_10m", 16_000_000, 70, 70), ("squelch", 4_000_000, 30, 6),
    ("junk", 5_000_000, 6, 2), ("cfo_spread", 6_250_000, 9, 5), ("frame_lengths", 3_000_000, 9, 5)])
def test_scenes_at_another_rate_lie_behind_the_priming_frames(name, fs, min_bursts, min_demods):
    """Called with another fs, a scene used to put its bursts at 530 * 2048 + <sample counts for 2 MHz>: inside the priming
    frames of a larger FFT, where the oracle and the pipeline agree on ZERO bursts and a comparison checks nothing.  The
    rate-aware layout gives the oracle the scene's bursts at every rate; counts no lower than the default scene's."""
    got_fs, iq = scenes.ALL[name](fs=fs)
    assert got_fs == fs and len(iq) % 32768 == 0
    r = orc.run_stream(iq, fs)
    assert len(r.bursts) >= min_bursts and len(r.demods) >= min_demods, (len(r.bursts), len(r.demods))
    assert min(b.start for b in r.bursts) >= 512 * scenes.nfft_of(fs)
    if name == "too_long":
        assert sum(1 for b in r.bursts if b.stop - b.start > int(0.09 * fs)) >= 2
    if name == "many_active_10m":
        assert _peak_active(r.bursts) >= 70
    if name == "squelch":
        first = 530 * scenes.nfft_of(fs)
        early = [b for b in r.bursts if b.start < first + fs // 2]
        assert len(early) >= 30 and max(b.stop - b.start for b in early) < fs // 100      # the dumped wave


def test_squelch_scene_is_kept_to_small_rates():
    with pytest.raises(AssertionError):
        scenes.squelch(fs=8_000_000)
    with pytest.raises(AssertionError):
        scenes.too_long(fs=1_000_000)
