"""Numpy oracles of the log-mel front end (``wsae_logmel``).

The contract, restated (``include/wsae.h`` carries it in full):

* constants: ``n_fft = 400``, ``hop = 160``, 201 bins, ``n_mels`` 80 or 128; ``P`` samples (a multiple of 160, >= 480) give
  ``T = P / 160`` frames; the waveform is zero from its length to ``P``;
* frame ``t`` covers padded samples ``160 t .. 160 t + 399`` of the length-``P`` signal with 200 reflected samples at both
  ends (``np.pad(mode="reflect")`` around ``P``); padded sample ``q`` is signal sample ``reflect_index(q - 200, P)``;
* ``re[t][k]`` / ``im[t][k]``: ONE float32 ``fma`` chain over ``n = 0 .. 399`` of ``sample * basis[n][k]`` /
  ``basis[n][208 + k]`` - the window lives in the caller's float32 basis;
* ``power = fl(fl(re re) + fl(im im))``; ``mel[t][m]``: ONE float32 ``fma`` chain over ``k = 0 .. 200`` of
  ``power[t][k] * filt[k][m]``;
* ``v = log10f(mel)`` where ``mel > float32(1e-10)``, else exactly -10;
* per utterance, float32: ``M = max v``; ``v = max(v, M - 8)``; ``out = (v + 4) / 4``.

``ideal`` is the same pipeline in float64 with the package's own tables (what the installed extractor's numpy path
computes); ``mirror`` evaluates the contract in float64 ON THE FLOAT32 TABLES the kernel gets and returns a bound for every
cell on what a conforming float32 implementation may deviate from it.
"""

from __future__ import annotations

import numpy as np

N_FFT, HOP, N_BINS, COLS, SIN_COL = 400, 160, 201, 416, 208
U = 2.0 ** -24          # float32 unit roundoff
FLOOR32 = float(np.float32(1e-10))
LOG10F_ULPS = 2.0       # the accuracy HIP documents for the device's log10f


def reflect_index(s, P):
    """Signal index behind index ``s`` of the signal extended by reflection (``-200 <= s < P + 200``)."""
    s = np.asarray(s, dtype=np.int64)
    return np.where(s < 0, -s, np.where(s >= P, 2 * (P - 1) - s, s))


def frames_of(wave, P):
    """``[T, 400]``: the frames of ``wave`` (1-D, at most ``P`` samples; zero up to ``P``), dtype kept."""
    wave = np.asarray(wave)
    if wave.ndim != 1 or wave.shape[0] > P or P % HOP or P < 3 * HOP:
        raise ValueError(f"need a 1-D waveform of at most P = {P} samples, P a multiple of {HOP} and >= {3 * HOP}")
    full = np.zeros(P, dtype=wave.dtype)
    full[:wave.shape[0]] = wave
    q = HOP * np.arange(P // HOP)[:, None] + np.arange(N_FFT)[None, :]
    return full[reflect_index(q - N_FFT // 2, P)]


def tail32(v32):
    """The per-utterance tail in float32, the extractor's operation order."""
    v32 = np.asarray(v32, dtype=np.float32)
    v32 = np.maximum(v32, v32.max() - np.float32(8.0))
    return (v32 + np.float32(4.0)) / np.float32(4.0)


def ideal(wave, P, n_mels):
    """``[n_mels, T]`` float32: float64 throughout (Hann window, ``rfft``, ``|.|^2``, the package's filter bank,
    ``log10(max(., 1e-10))``), rounded to float32 after the log, the tail in float32."""
    from whisper_sae.data.audio import hann_window, mel_filter_bank

    frames = frames_of(np.asarray(wave, dtype=np.float64), P) * hann_window()[None, :]
    spec = np.fft.rfft(frames, axis=1)
    power = np.abs(spec) ** 2
    mel = power @ mel_filter_bank(n_mels)
    return tail32(np.log10(np.maximum(mel, 1e-10)).astype(np.float32).T)


def mirror(x, basis32, filt32, P):
    """The contract in float64 on the kernel's own float32 operands.  ``x``: the float32 samples (int16 already scaled by
    2^-15), ``basis32 [400, 416]``, ``filt32 [201, n_mels]`` (non-negative or not).  Returns ``(out, E_out, mel, E_mel)``,
    all float64 ``[n_mels, T]``: a conforming kernel has ``|out_kernel - out| <= E_out`` and ``|mel_power_kernel - mel| <=
    E_mel`` in EVERY cell.

    The bound, from the chain lengths (Higham, Accuracy and Stability, section 3.1: a chain of n fma's computes
    ``sum a_i b_i (1 + th_i)``, ``|th_i| <= g(n) = n u / (1 - n u)``, ``u = 2^-24``):

    * DFT: ``e_re = g(400) * sum_n |x b_cos|``, ``e_im`` likewise (this float64 evaluation's own error, below ``400 * 2^-52``
      of the same sum, is added to ``g``);
    * power: with ``R = |re| + e_re``, ``I = |im| + e_im`` the computed operands lie within ``R``, ``I``, so
      ``e_p = (R^2 + I^2 - p) + 2 u (1 + u) (R^2 + I^2) + 2^-148`` (the two products and the sum round once each; the last
      term covers products that underflow);
    * mel: ``e_m = sum_k e_p |f| + g(201) * sum_k (p + e_p) |f|``;
    * log: both sides clamp at the floor (1-Lipschitz), the float32 floor is within ``u * 1e-10`` of 1e-10, and ``log10`` has
      slope ``1 / (ln 10 * y)``: ``e_v = e_m' / (ln 10 * max(m_c - e_m', 1e-10 (1 - 2 u)))`` with ``e_m' = e_m + u * 1e-10``,
      plus ``LOG10F_ULPS`` ulps of the result (``ulp(v) <= 2^-23 |v|``);
    * maximum: the kernel's ``M`` is some ``v_kernel[c]``, so ``M - e_v[argmax] <= M_kernel <= max_c (v[c] + e_up[c])``, where
      ``e_up = log10((m_c + e_m') / m_c)`` (+ ulps) is how far a cell can deviate UPWARDS - the logarithm is concave, so
      this is far below ``e_v`` in a quiet cell, which therefore cannot pretend to be the maximum; ``e_M`` is the larger
      deviation, plus the rounding of ``M - 8`` (``u * |M - 8|``, ``e_M`` included);
    * clamp: ``|max(a', b') - max(a, b)| <= max(|a' - a|, |b' - b|)``, so ``e_c = max(e_v, e_M)``;
    * ``(v + 4) / 4``: one rounding of the sum (``u * (|v + 4| + e_c)``), the division by 4 is exact:
      ``E_out = (e_c + u * (|v + 4| + e_c)) / 4``.

    Nothing in it is fitted to an implementation's output."""
    x = np.asarray(x)
    basis32, filt32 = np.asarray(basis32), np.asarray(filt32)
    if x.dtype != np.float32 or basis32.dtype != np.float32 or filt32.dtype != np.float32:
        raise ValueError("mirror evaluates the contract on float32 operands")
    if basis32.shape != (N_FFT, COLS) or filt32.shape[0] != N_BINS:
        raise ValueError(f"basis must be [{N_FFT}, {COLS}], filt [{N_BINS}, n_mels]")
    fr = frames_of(x, P).astype(np.float64)
    cos_t = basis32[:, :N_BINS].astype(np.float64)
    sin_t = basis32[:, SIN_COL:SIN_COL + N_BINS].astype(np.float64)
    f = filt32.astype(np.float64)
    g400 = 400 * U / (1 - 400 * U) + 400 * 2.0 ** -52
    g201 = 201 * U / (1 - 201 * U) + 201 * 2.0 ** -52
    re, im = fr @ cos_t, fr @ sin_t
    e_re, e_im = g400 * (np.abs(fr) @ np.abs(cos_t)), g400 * (np.abs(fr) @ np.abs(sin_t))
    p = re * re + im * im
    hi = (np.abs(re) + e_re) ** 2 + (np.abs(im) + e_im) ** 2
    e_p = (hi - p) + 2 * U * (1 + U) * hi + 2.0 ** -148
    mel = p @ f
    e_m = e_p @ np.abs(f) + g201 * ((p + e_p) @ np.abs(f))
    m_c = np.maximum(mel, 1e-10)
    v = np.log10(m_c)
    e_m1 = e_m + U * 1e-10
    e_v = e_m1 / (np.log(10.0) * np.maximum(m_c - e_m1, 1e-10 * (1 - 2 * U)))
    e_v = e_v + LOG10F_ULPS * 2.0 ** -23 * (np.abs(v) + e_v)
    e_up = np.log10((m_c + e_m1) / m_c)
    e_up = e_up + LOG10F_ULPS * 2.0 ** -23 * (np.abs(v) + e_up)
    big = v.max()
    at = np.unravel_index(np.argmax(v), v.shape)
    e_big = max(e_v[at], (v + e_up).max() - big)
    e_big = e_big + U * (abs(big - 8.0) + e_big)
    v2 = np.maximum(v, big - 8.0)
    e_c = np.maximum(e_v, e_big)
    out = (v2 + 4.0) / 4.0
    e_out = (e_c + U * (np.abs(v2 + 4.0) + e_c)) / 4.0
    return out.T.copy(), e_out.T.copy(), mel.T.copy(), e_m.T.copy()


def signals(P, seed=0):
    """The test signals, float64 ``[P]`` each: white noise; a 440 Hz tone followed by digital silence and faint noise; an
    amplitude-modulated 120 Hz tone with noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(P) / 16000.0
    noise = 0.3 * rng.standard_normal(P)
    tone = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    third = P // 3
    tone[third:2 * third] = 0.0
    tone[2 * third:] = 1e-4 * rng.standard_normal(P - 2 * third)
    am = 0.4 * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * 120.0 * t) + 0.01 * rng.standard_normal(P)
    return {"noise": np.clip(noise, -1.0, 1.0), "tone_silence": tone, "am_tone": np.clip(am, -1.0, 1.0)}


def integer_tables(n_mels, seed=1):
    """An integer basis ``[400, 416]`` with entries in -1..1, every column different and no symmetry between the cosine and
    the sine half, and a sparse integer filter bank ``[201, n_mels]`` (at most three bins of weight 1 or 2 per mel row):
    with samples in -1..1 (or halves) every intermediate is an integer (a multiple of 1/4) below 2^24 / 4, so float32
    computes it exactly in any order."""
    rng = np.random.default_rng(seed)
    basis = np.zeros((N_FFT, COLS), dtype=np.float32)
    cols = np.r_[0:N_BINS, SIN_COL:SIN_COL + N_BINS]
    basis[:, cols] = rng.integers(-1, 2, size=(N_FFT, cols.size)).astype(np.float32)
    assert np.unique(basis[:, cols], axis=1).shape[1] == cols.size
    filt = np.zeros((N_BINS, n_mels), dtype=np.float32)
    for m in range(n_mels):
        bins = rng.choice(N_BINS, size=3, replace=False)
        filt[bins, m] = rng.integers(1, 3, size=3)
    filt[N_BINS - 1, 0] = 2.0  # the last bin (the K tail of the contraction) is used
    filt[0, n_mels - 1] = 1.0
    return basis, filt


def integer_mel_power(x, basis, filt, P):
    """``[n_mels, T]`` float64, exact: ``x`` holds multiples of 1/2 in -1..1."""
    fr = frames_of(np.asarray(x, dtype=np.float64), P)
    re = fr @ basis[:, :N_BINS].astype(np.float64)
    im = fr @ basis[:, SIN_COL:SIN_COL + N_BINS].astype(np.float64)
    mel = (re * re + im * im) @ filt.astype(np.float64)
    assert mel.max() * 4 < 2 ** 24 and np.all(mel * 4 == np.round(mel * 4))
    return mel.T.copy()
