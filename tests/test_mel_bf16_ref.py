"""The split-bf16 reference (tests/mel_bf16_ref.py) against the float64 reference of the full
product (tests/mel_ref.py), without a GPU: on test_mel.py's configurations and signal families the
kept-term sums stay within the truncation bounds the header states, T6 = 3 * 2^-24 S and
T3 = 2^-14 S with S = sum_n |c| |x|, propagated through P and v as mel_ref propagates its e_re."""
import numpy as np
import pytest

from . import mel_bf16_ref as bref
from . import mel_ref as ref
from .test_mel import CONFIGS, filters_of, signals


def test_rounding_and_pieces():
    v = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF818000, 0, 0x3EAAAAAB], dtype=np.uint32).view(np.float32)
    want = np.array([0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF82, 0, 0x3EAB], dtype=np.uint32) << 16
    assert np.array_equal(bref.bf16(v).view(np.uint32), want)  # ties to even, both ways
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-1, 1, 4096), rng.integers(-32768, 32768, 4096) / 32768.0, [1.0, -1.0, 0.0, 2.0 ** 64]])
    p = bref.pieces(x.astype(np.float32))
    assert np.array_equal(p.sum(axis=0), x.astype(np.float32).astype(np.float64))
    assert not p[2][4096:8192].any()  # a 16-bit sample is exact in two pieces
    assert (np.abs(p[1]) <= 2.0 ** -8 * np.abs(p[0])).all() and (np.abs(p[2]) <= 2.0 ** -16 * np.abs(p[0])).all()


@pytest.mark.parametrize("N,hop,n_bins,center", CONFIGS)
def test_truncation_stays_within_its_bound(N, hop, n_bins, center):
    rng = np.random.default_rng(N * 7 + hop)
    T = 40 * hop + 77
    w = ref.hann(N) if N > 2 else np.array([0.75, 1.0], np.float32)
    F = filters_of(rng, n_bins, N // 2 + 1)
    sig = signals(rng, N, hop, T)
    frames = min(ref.mel_frames(T, N, hop, center) + 2, 12)
    x = np.stack(list(sig.values())).astype(np.float32)
    full, _ = ref.features(x, w, F, hop, center, 0, frames)
    err = {}
    for terms in (6, 3):
        v, e_v = bref.features(x, w, F, hop, center, 0, frames, terms, bref.truncation_factor(terms))
        assert v.shape == full.shape and np.isfinite(v).all()
        d = np.abs(v - full)
        assert (d[e_v == 0] == 0).all()
        ratio = float((d[e_v > 0] / e_v[e_v > 0]).max())
        print(f"{N, hop, n_bins, center} terms {terms}: worst |kept - full| / bound = {ratio:.4f}")
        assert ratio <= 1.0
        err[terms] = d
        zero = list(sig).index("zero")
        assert not v[zero].any()
    noise = list(sig).index("noise")
    assert err[6][noise].max() < err[3][noise].max()  # the six-term form is the closer one
