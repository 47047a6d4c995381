"""Audio clip export on the MI355X: ``wsae_clip_extract`` through the C ABI - junk tails behind every
array, junk beyond every length and between the rows, a sentinel in every output cell the kernel must not write, a
poisoned workspace - bit for bit equal to tests/clip_oracle.py, and the Python layer up to the WAV files of
``AudioClipExtractor.extract_all_clips``.  The oracle itself is checked against the reference's clips on the CPU in
tests/test_audio_clips.py."""

from __future__ import annotations

import json
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import clip_oracle as CO
from whisper_sae import _native as N
from whisper_sae.analysis import (AudioClipConfig, AudioClipExtractor, FeatureActivation, FeatureReport, RunTracker, TopKTracker,
                                  WaveformBank, clip_table_for_events, cut_clips)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 5  # junk elements behind every array
T = N.CLIP_TILE
GOLDEN = Path(__file__).resolve().parent / "golden"
JUNK = {np.dtype(np.float32): np.float32(3.0e4), np.dtype(np.int16): np.int16(-12345)}
SENTINEL = {np.dtype(np.float32): np.float32(7.5), np.dtype(np.int16): np.int16(0x5A5A)}
CODE = {np.dtype(np.float32): N.DT_F32, np.dtype(np.int16): N.DT_I16}
DTYPES = (np.float32, np.int16)


def padded(a: np.ndarray, junk) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    return torch.cat((t, torch.full((TAIL,), junk, dtype=t.dtype))).to(DEV)


def run_clips(x, lengths, utt, start, count, off, *, max_count, out_elems, out_dtype, gain, target=0.95, fade=0, ld_x=None,
              max_length=None, peak=True, x_skew=0, out_skew=0):
    """``wsae_clip_extract`` on ``x [n_utt, S]`` -> ``(out [out_elems], out_len, out_peak)`` as numpy, each checked against
    the oracle bit for bit, the sentinels included.  The rows of ``x`` have stride ``ld_x`` with junk between, behind and
    from each length on; ``x_skew`` / ``out_skew`` shift the two base pointers by that many elements off their allocation's
    alignment."""
    n_utt, s = x.shape
    n_clips = len(utt)
    ld_x = s if ld_x is None else ld_x
    max_length = s if max_length is None else max_length
    junk = JUNK[x.dtype]
    rows = np.full((n_utt, ld_x), junk, dtype=x.dtype)
    rows[:, :s] = x
    for u, n in enumerate(lengths):  # nothing at or beyond the length is read: junk there too
        rows[u, max(min(int(n), max_length), 0):] = junk
    dx = padded(np.concatenate((np.full(x_skew, junk, x.dtype), rows.reshape(-1))), junk)
    dl = padded(np.asarray(lengths, np.int32), 0x5A5A5A5)
    du, dc = padded(np.asarray(utt, np.int32), 0), padded(np.asarray(count, np.int32), 1 << 20)
    ds, do = padded(np.asarray(start, np.int64), 0), padded(np.asarray(off, np.int64), 0)
    out_dtype = np.dtype(out_dtype)
    before = np.full(out_skew + out_elems + TAIL, SENTINEL[out_dtype], out_dtype)
    out = torch.from_numpy(before).to(DEV)
    d_len = torch.full((n_clips + TAIL,), -77, dtype=torch.int32, device=DEV)
    d_peak = torch.full((n_clips + TAIL,), -3.5, dtype=torch.float32, device=DEV) if peak else None
    lib = N.lib()
    need = lib.wsae_clip_workspace_bytes(n_clips, max_count)
    assert need >= 0
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)  # (NaNs on entry)
    N.check(lib.wsae_clip_extract(dx.data_ptr() + x_skew * x.dtype.itemsize, CODE[x.dtype], n_utt, ld_x, dl.data_ptr(), max_length,
                                  n_clips, du.data_ptr(), ds.data_ptr(), dc.data_ptr(), max_count, do.data_ptr(), gain, target, fade,
                                  out.data_ptr() + out_skew * out_dtype.itemsize, CODE[out_dtype], out_elems, d_len.data_ptr(),
                                  N.ptr(d_peak), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "wsae_clip_extract")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xFF).all()), "the workspace's tail was written"
    got = out.cpu().numpy()
    assert (got[:out_skew] == SENTINEL[out_dtype]).all() and (got[out_skew + out_elems:] == SENTINEL[out_dtype]).all()
    got = got[out_skew:out_skew + out_elems]
    want, want_len, want_peak = CO.extract(x, lengths, max_length, utt, start, count, max_count, off, gain, target, fade,
                                           before[:out_elems])
    bits = np.uint32 if out_dtype == np.float32 else np.uint16
    wrong = np.flatnonzero(got.view(bits) != want.view(bits))
    assert wrong.size == 0, f"{wrong.size} cells differ, the first at {wrong[:5]}: {got[wrong[:5]]} for {want[wrong[:5]]}"
    got_len = d_len.cpu().numpy()
    assert (got_len[n_clips:] == -77).all() and np.array_equal(got_len[:n_clips], want_len)
    got_peak = None
    if peak:
        got_peak = d_peak.cpu().numpy()
        assert (got_peak[n_clips:] == -3.5).all()
        got_peak = got_peak[:n_clips]
        assert np.array_equal(got_peak.view(np.uint32), want_peak.view(np.uint32))
    return got, got_len[:n_clips], got_peak


def waveforms(dtype, n_utt, s, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32768, 32768, size=(n_utt, s)).astype(np.int16)
    return rng.uniform(-1.0, 1.0, size=(n_utt, s)).astype(np.float32)


S = 2 * T + 40
MAXC = 2 * T + 5
LENGTHS = [S, 0, S + 100, 5000]  # full, empty, above max_length (clamped to it), short with junk behind
# (utt, start, count): every count at which the code takes another path, at odd starts; the clamps at either end
TABLE = [(0, 1, 0), (0, 3, 1), (0, 17, 3), (0, 5, T - 1), (0, 8, T), (0, 2, T + 1), (0, 11, 2 * T + 5),
         (0, 7, 3 * T),            # count > max_count
         (0, -50, 100),            # start negative: moved to 0, keeps its count
         (0, S + 5, 10),           # start beyond the length
         (3, 4990, 100),           # end beyond the length
         (1, 0, 64),               # length 0
         (2, S - 10, 100),         # length above max_length
         (-1, 0, 10), (4, 0, 10),  # clip_utt out of range
         (3, 100, 333), (3, 1000, 2 * T + 5), (2, 4097, 77)]


def offsets_for(table, lengths, max_length, max_count, gaps=(1, 3, 0, 5, 2, 8)):
    """Non-overlapping output ranges with gaps of changing parity; clip 4 starts on a 64-byte boundary."""
    off, at = [], 3
    for c, (u, s0, cnt) in enumerate(table):
        n = CO.bounds(s0, cnt, lengths[u], max_length, max_count)[1] if 0 <= u < len(lengths) else 0
        if c == 4:
            at = (at + 63) // 64 * 64
        off.append(at)
        at += n + gaps[c % len(gaps)]
    return off, at


# ---- the C ABI, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fade,gain", ((0, 1), (1, 1), (7, 1), (5000, 1), (0, 0), (7, 0)))
@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("x_dtype", DTYPES)
def test_every_count_and_clamp_is_exact(x_dtype, out_dtype, fade, gain):
    """18 clips over four utterances, ld_x > S and odd (rows start at odd element offsets), both base pointers skewed.  Two
    clips are then made invalid through clip_off.  (int16 -> int16, no gain, no fade is the plain copy.)"""
    x = waveforms(x_dtype, 4, S, seed=fade + 10 * gain)
    off, total = offsets_for(TABLE, LENGTHS, S, MAXC)
    utt, start, count = (list(col) for col in zip(*TABLE))
    off[15] = -3             # clip_off out of range: below 0 ...
    off[17] = total - 76     # ... and one cell too far (n = 77)
    got, got_len, _ = run_clips(x, LENGTHS, utt, start, count, off, max_count=MAXC, out_elems=total, out_dtype=out_dtype, gain=gain,
                                fade=fade, ld_x=S + 37, x_skew=1, out_skew=3)
    assert got_len.tolist() == [0, 1, 3, T - 1, T, T + 1, 2 * T + 5, 2 * T + 5, 100, 0, 10, 0, 10, -1, -1, -1, 4000, -1]


@pytest.mark.parametrize("n_clips", (0, 1, 7))
def test_clip_counts(n_clips):
    x = waveforms(np.float32, 4, S, seed=n_clips)
    table = TABLE[4:4 + n_clips]
    off, total = offsets_for(table, LENGTHS, S, MAXC)
    utt, start, count = (list(col) for col in zip(*table)) if table else ([], [], [])
    run_clips(x, LENGTHS, utt, start, count, off, max_count=MAXC, out_elems=total + 1, out_dtype=np.int16, gain=1, fade=3)


@pytest.mark.parametrize("x_dtype", DTYPES)
def test_peak_in_the_last_element_all_zero_clip_and_full_scale(x_dtype):
    """The peak of clip 0 is a negative sample in the last element of its last tile; clip 1 is all zero (no gain: zeros,
    peak 0); with target 1 and int16 output the peaks become exactly -32767 and +32767 and nothing clips."""
    n = 2 * T + 5
    x = (waveforms(x_dtype, 2, n + 20, seed=5) // 4 if x_dtype == np.int16 else waveforms(x_dtype, 2, n + 20, seed=5) / 4)
    x = x.astype(x_dtype)
    big = {np.float32: np.float32(0.9), np.int16: np.int16(30000)}[x_dtype]
    x[0, 3 + n - 1] = -big
    x[1, :3000] = 0
    x[1, 3000 + 123] = big
    table = [(0, 3, n), (1, 100, 2000), (1, 3000, T)]
    utt, start, count = (list(col) for col in zip(*table))
    off = [0, n + 11, n + 11 + 2000 + 5]
    total = off[2] + T
    for out_dtype in DTYPES:
        got, _, peak = run_clips(x, [n + 20] * 2, utt, start, count, off, max_count=n, out_elems=total, out_dtype=out_dtype, gain=1,
                                 target=1.0)
        want_peak = np.float32(0.9) if x_dtype == np.float32 else np.float32(30000 / 32768)
        assert peak.tolist() == [want_peak, 0.0, want_peak]
        full = {np.float32: np.float32(1.0), np.int16: np.int16(32767)}[out_dtype]
        assert got[n - 1] == -full and got[off[2] + 123] == full and np.abs(got[:n].astype(np.float64)).max() == full
        assert not got[off[1]:off[1] + 2000].any()


def test_montage_second_call_and_permuted_table():
    """One buffer with the clips in order and 11 cells of silence between them - the gaps keep the sentinel - then the
    same bits from a second call, without out_peak and with the table permuted."""
    x = waveforms(np.int16, 3, 6000, seed=9)
    lengths = [6000, 2500, 4100]
    table = [(0, 10, 3000), (1, 2000, 3000), (2, -7, 4100), (0, 5999, 3), (2, 4000, 4100), (1, 1, 1)]
    utt, start, count = (list(col) for col in zip(*table))
    ns = [CO.bounds(s, c, lengths[u], 6000, 4100)[1] for u, s, c in table]
    off = [int(v) for v in np.cumsum([0] + [n + 11 for n in ns[:-1]])]
    total = off[-1] + ns[-1]
    kw = dict(max_count=4100, out_elems=total, out_dtype=np.int16, gain=1, fade=16)
    first, first_len, first_peak = run_clips(x, lengths, utt, start, count, off, **kw)
    for c in range(len(table) - 1):
        assert (first[off[c] + ns[c]:off[c + 1]] == SENTINEL[np.dtype(np.int16)]).all()
    again, _, _ = run_clips(x, lengths, utt, start, count, off, peak=False, **kw)
    assert np.array_equal(first, again)
    order = [4, 0, 5, 2, 1, 3]
    pick = lambda v: [v[i] for i in order]
    shuffled, sh_len, sh_peak = run_clips(x, lengths, pick(utt), pick(start), pick(count), pick(off), **kw)
    assert np.array_equal(first, shuffled) and np.array_equal(first_len[order], sh_len)
    assert np.array_equal(first_peak[order].view(np.uint32), sh_peak.view(np.uint32))
    # no gain and no out_peak: the peak pass is not needed at all
    run_clips(x, lengths, utt, start, count, off, peak=False, **dict(kw, gain=0))


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_cut_clips_rows_and_montage_against_the_oracle():
    rng = np.random.default_rng(3)
    sizes = [5000, 1200, 9000]
    waves = [rng.uniform(-1, 1, size=n).astype(np.float32) for n in sizes]
    bank = WaveformBank([torch.from_numpy(w) for w in waves])  # CPU tensors of different lengths: packed on the device
    assert bank.n_utt == 3 and bank.max_length == 9000 and bank.lengths.tolist() == sizes and bank.dtype == torch.float32
    x = np.zeros((3, 9000), np.float32)
    for u, w in enumerate(waves):
        x[u, :len(w)] = w
    utt, start, count = [2, 0, 1, 2, 5], [100, -20, 1000, 8990, 0], [T + 3, 700, 500, 50, 10]
    for pcm in (False, True):
        dtype = np.int16 if pcm else np.float32
        rows = cut_clips(bank, utt, start, count, target=0.5, fade=8, pcm16=pcm)
        assert rows.samples.shape == (5, T + 3) and rows.offsets.tolist() == [c * (T + 3) for c in range(5)]
        want, want_len, want_peak = CO.extract(x, sizes, 9000, utt, start, count, T + 3, rows.offsets.tolist(), CO.GAIN_PEAK, 0.5, 8,
                                               np.zeros(5 * (T + 3), dtype))
        assert np.array_equal(rows.samples.cpu().numpy().reshape(-1), want) and rows.samples.cpu().numpy().dtype == dtype
        assert rows.lengths.tolist() == want_len.tolist() == [T + 3, 700, 200, 10, -1]
        assert np.array_equal(rows.peaks.cpu().numpy(), want_peak)
        tape = cut_clips(bank, torch.tensor(utt, device=DEV), torch.tensor(start, device=DEV), torch.tensor(count, device=DEV),
                         normalize=False, pcm16=pcm, layout="montage", gap=40, max_count=T + 3)
        ns = [T + 3, 700, 200, 10, 0]
        offs = [int(v) for v in np.cumsum([0] + [n + 40 for n in ns[:-1]])]
        assert tape.offsets.tolist() == offs and tape.samples.shape == (sum(ns) + 4 * 40,)
        want, want_len, _ = CO.extract(x, sizes, 9000, utt, start, count, T + 3, offs, CO.GAIN_NONE, 0.95, 0,
                                       np.zeros(sum(ns) + 160, dtype))
        assert np.array_equal(tape.samples.cpu().numpy(), want) and tape.lengths.tolist() == want_len.tolist()
    empty = cut_clips(bank, [], [], [])
    assert empty.samples.shape == (0, 0) and empty.lengths.numel() == 0
    assert bank._workspace is not None and bank._workspace.numel() * 4 >= N.lib().wsae_clip_workspace_bytes(5, T + 3)
    pcm_bank = WaveformBank(torch.tensor([[0, 16384, -32768, 5]], dtype=torch.int16), lengths=[3])
    got = cut_clips(pcm_bank, [0], [0], [4], normalize=False)
    assert got.samples.tolist() == [[0.0, 0.5, -1.0, 0.0]] and got.lengths.tolist() == [3] and got.peaks.tolist() == [1.0]


def golden_loader(sample_idx: int) -> torch.Tensor:
    wave_ = torch.from_numpy(CO.golden_waveform(sample_idx))
    return wave_.unsqueeze(0) if sample_idx == 2 else wave_


def test_extract_clip_equals_the_reference_clips_bit_for_bit(tmp_path):
    g = np.load(GOLDEN / "g20_audio_clips.npz")
    for norm in (0, 1):
        cfg = AudioClipConfig(clip_duration_ms=50.0, context_before_ms=25.0, normalize_audio=bool(norm))
        ex = AudioClipExtractor(TopKTracker(num_features=1, k=1), golden_loader, tmp_path / f"n{norm}", cfg, device=DEV)
        for name, u, p in g["cases"]:
            act = FeatureActivation(feature_idx=0, activation_value=1.0, sample_idx=int(u), position_idx=int(p))
            clip = ex.extract_clip(act) if name != "all_zero" else ex.extract_clip(act, golden_loader(1))
            assert clip.device.type == "cpu" and clip.dtype == torch.float32 and clip.dim() == 1
            key = f"n{norm}_{name}"
            if key in g.files:
                assert np.array_equal(clip.numpy().view(np.uint32), g[key].view(np.uint32)), key
            else:  # the reference raises on the empty clip; here it is empty
                assert key == "n1_beyond_end" and clip.numel() == 0
    broken = AudioClipExtractor(TopKTracker(num_features=1, k=1), lambda i: 1 / 0, tmp_path / "broken", device=DEV)
    assert broken.extract_clip(FeatureActivation(0, 1.0, 0, 0)) is None


def test_golden_tracker_end_to_end_writes_the_references_manifest(tmp_path):
    doc = json.loads((GOLDEN / "g20_manifest.json").read_text())
    (tmp_path / "state.json").write_text(json.dumps(doc["tracker_state"]))
    tracker = TopKTracker.load(tmp_path / "state.json")
    out = tmp_path / "clips"
    ex = AudioClipExtractor(tracker, golden_loader, out, AudioClipConfig(clip_duration_ms=50.0, context_before_ms=25.0), device=DEV)
    written = ex.extract_all_clips()
    assert {str(f): [str(p.relative_to(out)) for p in ps] for f, ps in written.items()} == doc["written"]
    manifest = json.loads(json.dumps(json.loads(ex.save_manifest().read_text())).replace(str(out) + "/", ""))
    assert manifest == doc["manifest"]
    report = FeatureReport(tracker, tmp_path / "reports", clips=ex).generate_feature_report(0)
    assert [Path(e["audio_path"]).relative_to(out).as_posix() for e in report["top_examples"]] == doc["written"]["0"]
    # the files hold the reference's floats as 16-bit PCM
    g = {u: CO.golden_waveform(u) for u in range(3)}
    for f, entries in doc["manifest"]["features"].items():
        for e in entries:
            s0, n = CO.bounds(e["position_idx"] * 160 - 400, 800, len(g[e["sample_idx"]]), 4000, 800)
            want, _ = CO.clip_values(g[e["sample_idx"]][s0:s0 + n], CO.GAIN_PEAK, 0.95, 0, True)
            assert np.array_equal(read_pcm(out / e["audio_path"]), want), e["audio_path"]


def read_pcm(path) -> np.ndarray:
    with wave.open(str(path), "rb") as fh:
        assert (fh.getnchannels(), fh.getsampwidth(), fh.getframerate()) == (1, 2, 16000)
        return np.frombuffer(fh.readframes(fh.getnframes()), "<i2")


@pytest.fixture(scope="module")
def tiny():
    """H = 8, k = 2, three utterances of 12 frames: the compact code, its tracker, and waveforms of 3000, 1200 and 900
    samples - the frames reach to 1920, so clips of the two short ones are cut by the end or empty."""
    H, K, FR = 8, 2, 12
    rng = np.random.default_rng(11)
    idx = np.stack([rng.permutation(H)[:K] for _ in range(3 * FR)]).astype(np.int32).reshape(3, FR, K)
    val = (rng.permutation(3 * FR * K).astype(np.float32) + 1).reshape(3, FR, K) / 8  # distinct, positive
    val[rng.uniform(size=val.shape) < 0.3] = 0
    waves = [rng.integers(-20000, 20000, size=n).astype(np.int16).astype(np.float32) / np.float32(32768) for n in (3000, 1200, 900)]
    return H, FR, torch.from_numpy(val).to(DEV), torch.from_numpy(idx).to(DEV), waves


def tiny_tracker(tiny) -> TopKTracker:
    H, FR, val, idx, _ = tiny
    tracker = TopKTracker(H, k=3, device=DEV)
    tracker.update_compact(val, idx, [0, 1, 2], seq_len=FR)
    return tracker


CFG = AudioClipConfig(clip_duration_ms=50.0, context_before_ms=25.0, fade_ms=1.0)


def check_files(ex, out, waves, skipped=()):
    """Every WAV under ``out`` against the oracle's PCM, the montages against the clips in rank order 160 zeros apart."""
    seen = 0
    for f in range(ex.tracker.num_features):
        pieces = []
        for rank, e in enumerate(ex.examples(f)):
            path = out / f"feature_{f:05d}" / f"rank{rank:02d}_act{e.activation_value:.3f}.wav"
            if e.sample_idx in skipped:
                assert not path.exists() and e.audio_path is None
                continue
            x = waves[e.sample_idx]
            s0, n = CO.bounds(e.position_idx * 160 - 400, 800, len(x), len(x), 800)
            want, _ = CO.clip_values(x[s0:s0 + n], CO.GAIN_PEAK, 0.95, 16, True)
            assert e.audio_path == str(path) and np.array_equal(read_pcm(path), want), path
            pieces += [np.zeros(160, np.int16), want] if pieces else [want]
            seen += 1
        montage = out / f"feature_{f:05d}" / "montage.wav"
        if pieces:
            assert np.array_equal(read_pcm(montage), np.concatenate(pieces)), montage
        else:
            assert not montage.exists()
    assert seen == len(list(out.glob("feature_*/rank*.wav"))) and seen > 0
    return seen


def test_extract_all_clips_end_to_end(tiny, tmp_path):
    waves = tiny[4]
    calls = []

    def loader(i):
        calls.append(i)
        return torch.from_numpy(waves[i])

    ex = AudioClipExtractor(tiny_tracker(tiny), loader, tmp_path / "a", CFG)
    progress = []
    written = ex.extract_all_clips(montage=True, gap_ms=10.0, progress_callback=lambda i, n: progress.append((i, n)))
    assert sorted(calls) == [0, 1, 2] and ex.loads == 3, "every utterance is loaded exactly once"
    seen = check_files(ex, tmp_path / "a", waves)
    assert sum(len(p) for p in written.values()) == seen and progress == [(i, len(written)) for i in range(len(written))]
    lengths = [len(read_pcm(p)) for ps in written.values() for p in ps]
    assert 800 in lengths and any(0 < n < 800 for n in lengths), "the fixture has whole and cut clips"
    manifest = json.loads(ex.save_manifest().read_text())
    assert sum(len(v) for v in manifest["features"].values()) == seen

    # chunks of one feature: the same files; a chunk loads what it cites, except what the chunk before it hands over
    calls.clear()
    small = AudioClipExtractor(tiny_tracker(tiny), loader, tmp_path / "b", CFG, bank_bytes=1)
    small.extract_all_clips(montage=True, gap_ms=10.0)
    want_calls, before = [], set()
    for f in range(8):
        cited = list(dict.fromkeys(e.sample_idx for e in small.examples(f)))
        if cited:
            want_calls += [s for s in cited if s not in before]
            before = set(cited)
    assert calls == want_calls and len(calls) > 3
    for a in sorted((tmp_path / "a").glob("feature_*/*.wav")):
        assert (tmp_path / "b" / a.relative_to(tmp_path / "a")).read_bytes() == a.read_bytes()

    # one feature alone, two clips at most
    one = AudioClipExtractor(tiny_tracker(tiny), loader, tmp_path / "c", CFG)
    f = next(iter(written))
    paths = one.extract_feature_clips(f, max_clips=2)
    assert [p.name for p in paths] == [p.name for p in written[f][:2]] and not (tmp_path / "c" / f"feature_{f:05d}" / "montage.wav").exists()


def test_a_raising_loader_costs_only_its_own_clips(tiny, tmp_path, capsys):
    waves = tiny[4]
    calls = []

    def loader(i):
        calls.append(i)
        if i == 1:
            raise OSError("no such file")
        return torch.from_numpy(waves[i]).unsqueeze(0)  # [1, n]

    ex = AudioClipExtractor(tiny_tracker(tiny), loader, tmp_path, CFG)
    ex.extract_all_clips(montage=True, gap_ms=10.0)
    assert sorted(calls) == [0, 1, 2]
    assert "Failed to load audio for sample 1: no such file" in capsys.readouterr().out
    check_files(ex, tmp_path, waves, skipped=(1,))


def test_event_clips_have_the_bounds_of_sample_bounds(tiny):
    H, FR, val, idx, _ = tiny
    runs = RunTracker(H, max_events=3 * FR * 2, device=DEV)
    runs.update((val, idx))
    ev = runs.events()
    n_ev = ev.feature.numel()
    assert n_ev > 8
    rng = np.random.default_rng(2)
    lengths = [FR * 320, FR * 320 - 100, 5 * 320 + 7]  # whole, a little short, much shorter than the frames
    x = rng.uniform(-1, 1, size=(3, FR * 320)).astype(np.float32)
    bank = WaveformBank(torch.from_numpy(x), lengths=lengths)
    for ctx in (0, 1):
        utt, start, count = clip_table_for_events(ev, context_frames=ctx)
        lo, hi = ev.sample_bounds(320, ctx)
        assert torch.equal(start, lo) and torch.equal(start + count, hi) and utt.device.type == "cuda"
        batch = cut_clips(bank, utt, start, count, normalize=False)
        L = torch.tensor(lengths, device=DEV)[ev.utterance.long()]
        assert torch.equal(batch.lengths.long(), (torch.minimum(hi, L) - lo).clamp(min=0))
        got, n, lo_h, u_h = batch.samples.cpu().numpy(), batch.lengths.cpu().numpy(), lo.cpu().numpy(), utt.cpu().numpy()
        for c in range(n_ev):
            assert np.array_equal(got[c, :n[c]], x[u_h[c], lo_h[c]:lo_h[c] + n[c]]) and not got[c, n[c]:].any()
    assert (ev.start == 0).any() and (ev.start + ev.length == FR).any(), "runs at frame 0 and at the last frame"
