"""The resampler without a GPU: the float32 fused multiply-add of tests/resample_oracle.py against exact rationals, the tap
tables against the values and properties they must have, the polyphase indexing against ``scipy.signal.upfirdn``, the exact
oracle against the float64 formulation within a derived bound, two properties of the filter itself, every argument error of
``wsae_resample`` (found on the host before any HIP call) and the errors of the Python layer."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import resample_oracle as RO
from whisper_sae import _native as N
from whisper_sae.data import AudioFrontEnd, Resampler, compact_taps, resample, resampled_length, sinc_resample_kernel

U = 2.0 ** -24  # unit roundoff of float32


def round_to_f32(q: Fraction) -> float:
    """The float32 nearest to the rational ``q``, ties to even (normal range)."""
    if q == 0:
        return 0.0
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 24
    while q / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while q / Fraction(2) ** e < 2 ** 23:
        e -= 1
    scaled = q / Fraction(2) ** e
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * math.ldexp(n, e)


def test_fma32_is_correctly_rounded_on_random_triples():
    rng = np.random.default_rng(0)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n)).astype(np.float32)
    near = rng.random(n) < 0.5  # half of them cancel: c close to -a b, where the low bits of the product decide
    c[near] = (-(a[near].astype(np.float64) * b[near]) * (1 + rng.integers(-3, 4, near.sum()) * 2.0 ** -22)).astype(np.float32)
    got = RO.fma32(a, b, c)
    want = np.array([round_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma32_on_constructed_ties():
    """``a b`` exactly halfway between two float32, the lower of them even ((1 + 2^-12)^2) and odd ((1 + 2^-12)(1 + 3 2^-12));
    then nudged off the tie by a ``c`` far below the float64 sum's last bit, which a double rounding would lose."""
    one = np.float32(1)
    x1, x3 = np.float32(1 + 2.0 ** -12), np.float32(1 + 3 * 2.0 ** -12)
    ulp = np.float32(2.0 ** -23)
    tiny = np.float32(2.0 ** -60)
    lo_even, lo_odd = np.float32(1 + 2.0 ** -11), np.float32(1 + 2.0 ** -10 + 2.0 ** -23)
    assert int(lo_even.view(np.uint32)) % 2 == 0 and int(lo_odd.view(np.uint32)) % 2 == 1
    cases = ((x1, x1, 0.0, lo_even), (x1, x3, 0.0, lo_odd + ulp),           # exact ties: to even
             (x1, x1, tiny, lo_even + ulp), (x1, x1, -tiny, lo_even),        # just above / below the tie
             (x1, x3, tiny, lo_odd + ulp), (x1, x3, -tiny, lo_odd),
             (x1, x1, ulp, lo_even + ulp + ulp), (-x1, x1, 0.0, -lo_even), (-x1, x3, tiny, -lo_odd), (one, one, tiny, one))
    for a, b, c, want in cases:
        got = RO.fma32(np.float32(a), np.float32(b), np.float32(c))
        exact = round_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(np.float32(c))))
        assert float(got) == float(np.float32(want)) == exact, (a, b, c, float(got), exact)


TABLE = ((48000, 3, 1, 19, 37), (44100, 441, 160, 17, 34), (8000, 1, 2, 7, 13), (11025, 441, 640, 7, 13), (22050, 441, 320, 9, 17),
         (24000, 3, 2, 10, 19), (96000, 6, 1, 37, 73), (32000, 2, 1, 13, 25))


@pytest.mark.parametrize("rate,orig,new,width,W", TABLE)
def test_table_values_and_compaction(rate, orig, new, width, W):
    kernel, got_width = sinc_resample_kernel(rate, 16000)
    assert kernel.dtype == np.float64 and kernel.shape == (new, 2 * width + orig) and got_width == width
    taps, first, halo = compact_taps(kernel, width)
    assert taps.dtype == np.float32 and taps.shape == (new, W) and first.dtype == np.int32 and first.shape == (new,) and halo == width
    # nothing is lost: the taps scattered back by first are the float32 kernel, and the halo promise holds
    back = np.zeros(kernel.shape, np.float32)
    for p in range(new):
        back[p, first[p] + width:first[p] + width + W] = taps[p]
    assert np.array_equal(back, kernel.astype(np.float32))
    assert (first >= -halo).all() and (first + W <= orig + halo).all()
    assert abs(kernel.sum() / new - 1.0) < 1e-2  # unit gain at 0 Hz, up to what the window takes


def test_equal_rates_are_the_identity_table_and_wrong_arguments_raise():
    assert resampled_length(0, 48000) == 0 and resampled_length(1, 48000) == 1 and resampled_length(3, 48000) == 1
    for n in (0, 1, 2, 440, 441, 442, 1323000, 2 ** 31 - 1):
        for orig, new in ((44100, 16000), (8000, 16000), (16000, 16000), (11025, 16000)):
            assert resampled_length(n, orig, new) == (n * new + orig - 1) // orig
    with pytest.raises(ValueError, match="n must not be negative"):
        resampled_length(-1, 48000)
    with pytest.raises(ValueError, match="rates must be positive integers"):
        resampled_length(5, 0)
    with pytest.raises(ValueError, match="rates must be positive integers"):
        Resampler(44100.5)
    with pytest.raises(ValueError, match="16001 / 16000: both must be at most 1024"):
        Resampler(16001)
    with pytest.raises(ValueError, match="taps per phase"):
        Resampler(1021, 2)
    with pytest.raises(ValueError, match="lowpass_filter_width must be positive"):
        sinc_resample_kernel(48000, 16000, 0)
    with pytest.raises(ValueError, match="rolloff"):
        sinc_resample_kernel(48000, 16000, 6, 1.5)
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        Resampler(48000, device="cpu")
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        resample(torch.zeros(2, 480), 48000)
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        AudioFrontEnd(48000, device="cpu")
    with pytest.raises(ValueError, match="n_mels must be 80 or 128"):
        AudioFrontEnd(48000, n_mels=64)


@pytest.mark.parametrize("orig_freq,new_freq", ((48000, 16000), (44100, 16000), (8000, 16000)))
def test_polyphase_indexing_against_upfirdn(orig_freq, new_freq):
    from scipy.signal import upfirdn
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    kernel, width = sinc_resample_kernel(orig_freq, new_freq)
    K = kernel.shape[1]
    S = -(-(K - 1) // orig)
    h = np.zeros((new - 1) * orig + S * orig * new + 1)
    seen = np.zeros(h.size, bool)
    for p in range(new):
        idx = p * orig - np.arange(K) * new + S * orig * new
        assert (idx >= 0).all() and not seen[idx].any()  # the map is injective: orig and new are coprime
        h[idx], seen[idx] = kernel[p], True
    x = np.random.default_rng(3).standard_normal(3001)
    want = RO.resample_ideal(x, orig_freq, new_freq)
    xin = np.concatenate((np.zeros(width), x, np.zeros(K + orig)))
    got = upfirdn(h, xin, up=new, down=orig)[S * new:S * new + want.size]
    assert got.size == want.size == resampled_length(x.size, orig_freq, new_freq)
    eps = K * 2.0 ** -53
    bound = 2 * eps / (1 - eps) * RO.dense_apply(np.abs(kernel), width, np.abs(x), orig, new)
    print(f"{orig}/{new}: max |upfirdn - ideal| = {np.abs(got - want).max():.2e}, max ratio to the bound {np.max(np.abs(got - want) / bound):.3f}")
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("orig_freq", (48000, 44100, 8000, 11025, 96000))
def test_exact_oracle_is_within_the_derived_bound_of_the_ideal(orig_freq):
    """Per cell ``g(W) sum |x| |taps| + sum |x| |taps32 - k|`` with ``g(n) = n u / (1 - n u)``: the chain's rounding and the
    rounding of the table - derived, not fitted."""
    g = math.gcd(orig_freq, 16000)
    orig, new = orig_freq // g, 16000 // g
    kernel, width = sinc_resample_kernel(orig_freq, 16000)
    taps, first, _ = compact_taps(kernel, width)
    x = (np.random.default_rng(orig_freq).standard_normal(3 * orig * 5 + 7) * 0.3).astype(np.float32)
    got = RO.resample_exact(x, 1, x.size, orig, new, taps, first, np.float32)
    want = RO.resample_ideal(x, orig_freq, 16000)
    assert got.dtype == np.float32 and got.size == want.size
    W = taps.shape[1]
    k32 = kernel.astype(np.float32).astype(np.float64)
    gw = W * U / (1 - W * U)
    bound = gw * RO.dense_apply(np.abs(k32), width, np.abs(x), orig, new) + RO.dense_apply(np.abs(k32 - kernel), width, np.abs(x), orig, new)
    delta = np.abs(got.astype(np.float64) - want)
    print(f"{orig}/{new}: max |exact - ideal| = {delta.max():.2e}, max ratio to the bound {np.max(delta / bound):.3f}")
    assert (delta <= bound).all()


def test_exact_oracle_downmix_lengths_and_int16_rule():
    taps, first = np.ones((1, 1), np.float32), np.zeros(1, np.int32)
    x = np.array([100, 201, -32768, -32768, 32767, 32767, 1, 2, 9, 9], np.int16)
    y = RO.resample_exact(x, 2, 4, 1, 1, taps, first, np.float32)  # four frames of stereo; the fifth is not read
    assert np.array_equal(y, np.array([150.5, -32768, 32767, 1.5], np.float32) / np.float32(32768))
    y16 = RO.resample_exact(x, 2, 4, 1, 1, taps, first, np.int16)
    assert y16.dtype == np.int16 and y16.tolist() == [150, -32768, 32767, 2]  # halves to even
    three = RO.downmix(np.array([0.1, 0.2, 0.4], np.float32), 3)
    assert three[0] == (np.float32(0.1) + np.float32(0.2) + np.float32(0.4)) / np.float32(3)
    k, w = sinc_resample_kernel(8000, 16000)
    t, f, _ = compact_taps(k, w)
    for n in (0, 1, 5):
        assert RO.resample_exact(np.ones(5, np.float32), 1, n, 1, 2, t, f, np.float32).size == 2 * n


def test_filter_passes_1_khz_and_stops_12_khz_at_48_to_16():
    """Properties of torchaudio's default filter, not of this code: they catch a wrong scale or cut-off."""
    n = np.arange(48000)
    tone = RO.resample_ideal(np.sin(2 * np.pi * 1000 * n / 48000), 48000, 16000)
    ideal = np.sin(2 * np.pi * 1000 * np.arange(16000) / 16000)
    err = np.abs(tone - ideal)[200:15800].max()
    alias = RO.resample_ideal(np.sin(2 * np.pi * 12000 * n / 48000), 48000, 16000)[200:15800]
    rms = float(np.sqrt(np.mean(alias ** 2)))
    print(f"1 kHz: max error {err:.3e}; 12 kHz: rms {rms:.5f}")
    assert tone.size == 16000 and err < 1e-3 and rms < 0.01


def test_argument_errors_do_not_need_a_gpu():
    lib = N.lib()
    A = 0x1000  # any non-null aligned address: an argument error returns before anything is read
    # 0 x, 1 x_dtype, 2 n_utt, 3 ld_x, 4 channels, 5 length, 6 max_length, 7 orig, 8 new_, 9 taps, 10 first, 11 n_taps, 12 halo,
    # 13 out, 14 out_dtype, 15 ld_y, 16 out_cols, 17 out_len, 18 stream
    good = [A, N.DT_F32, 2, 3000, 1, A, 3000, 3, 1, A, A, 37, 19, A, N.DT_F32, 1000, 1000, A, None]
    cases = (({0: None}, "null"), ({5: None}, "null"), ({9: None}, "null"), ({10: None}, "null"), ({13: None}, "null"),
             ({17: None}, "null"), ({1: 1}, "x_dtype"), ({1: 7}, "x_dtype"), ({14: 1}, "out_dtype"), ({14: -1}, "out_dtype"),
             ({2: -1}, "n_utt"), ({4: 0}, "channels"), ({4: 9}, "channels"), ({4: 2}, "ld_x"), ({3: 2999}, "ld_x"),
             ({7: 0}, "orig"), ({7: 1025}, "orig"), ({8: 0}, "new_"), ({8: 1025}, "new_"), ({7: 6, 8: 3}, "coprime"),
             ({7: 4, 8: 2, 16: 1500, 15: 1500}, "coprime"), ({11: 0}, "n_taps"), ({11: 513}, "n_taps"), ({12: -1}, "halo"),
             ({12: 4097}, "halo"), ({11: 42}, "n_taps"), ({6: -1}, "max_length"), ({6: 2 ** 31, 3: 2 ** 31}, "max_length"),
             ({16: 999}, "out_cols"), ({16: 1001}, "ld_y"), ({15: 999}, "ld_y"), ({16: 2 ** 31, 15: 2 ** 31}, "out_cols"),
             ({0: A + 2}, "aligned"), ({9: A + 2}, "aligned"))
    for change, word in cases:
        args = list(good)
        for pos, bad in change.items():
            args[pos] = bad
        assert lib.wsae_resample(*args) == -1, change
        assert "wsae_resample" in N.last_error() and word in N.last_error(), (change, N.last_error())
    assert lib.wsae_resample(*good[:2], 0, *good[3:]) == 0  # no utterances: nothing is touched
    assert N.RESAMPLE_TILE % 256 == 0 and N.RESAMPLE_LDS_BYTES <= 160 * 1024
