"""The host-side argument checks that the analysis entry points share (``CW_REQUIRE_*`` in csrc/wsae_codewalk.h), seen
from outside and without a GPU: the WHOLE text of ``wsae_last_error()`` for every shared requirement of every entry point
that makes it, and, with two mistakes in one call, which of the two messages the caller gets - the order of the checks.
Host buffers stand in for the device pointers: a rejected call launches nothing and never follows them.  Apart from the
cases that leave the workspace pointer out, which a call with rows alone rejects, the calls have no rows, so that even an
accepted call would launch nothing.  Also here: the entry bound of ``wsae_feature_topk_update`` and the workspace sizes of the
analyses that build per-key lists (csrc/wsae_lists.h), pinned as literals."""

from __future__ import annotations

import ctypes

import pytest

from whisper_sae import _native as N

BUF = (ctypes.c_double * 64)()
P = ctypes.addressof(BUF)  # 8-byte aligned
BIG = 1 << 20


def probe_plan(k=8, hidden=96, n_rows=0, col_of=None, n_cols=96, t_row=P, t_val=P, cap=8, ws=P, ws_bytes=BIG):
    return N.lib().wsae_probe_plan(P, P, k, hidden, None, n_rows, col_of, n_cols, P, t_row, t_val, cap, P, ws, ws_bytes, None)


def probe_forward(k=8, hidden=96, n_rows=0, lag=0, C=3, col_of=None, n_cols=96, ldw=3):
    return N.lib().wsae_probe_forward(P, P, k, hidden, None, P, n_rows, lag, C, col_of, n_cols, P, ldw, P, None, None, 3, None, P,
                                      P, P, None, None, 0, None)


def probe_backward(t_row=P, t_val=P, cap=8, n_cols=96, lde=3, C=3, n_rows=0, ws=P, ws_bytes=BIG):
    return N.lib().wsae_probe_backward(P, t_row, t_val, cap, n_cols, P, lde, C, n_rows, P, P, ws, ws_bytes, None)


def gram_update(k=8, hidden=96, n_rows=0, col_of=None, n_cols=96, t_row=P, t_val=P, cap=8, p_rows=96, ws=P, ws_bytes=BIG):
    return N.lib().wsae_gram_update(P, P, k, hidden, None, n_rows, col_of, n_cols, P, t_row, t_val, cap, 0, p_rows, P, 96, ws,
                                    ws_bytes, None)


def regress_forward(k=8, hidden=96, n_rows=0, lag=0, C=3, col_of=None, n_cols=96, ldw=3, ws=P, ws_bytes=BIG):
    return N.lib().wsae_regress_forward(P, P, k, hidden, None, P, 3, n_rows, lag, C, col_of, n_cols, P, ldw, P, P, 3, P, P, ws,
                                        ws_bytes, None)


def label_update(k=8, hidden=96, n_rows=0, C=3, lags=(0, 0), f_cols=96):
    return N.lib().wsae_label_update(P, P, k, hidden, None, P, n_rows, C, lags[0], lags[1], 0, f_cols, None, 1, P, P, None, 0, None)


def sta_update(k=8, hidden=96, n_rows=0, channels=4, lags=(-1, 1), f_cols=96, ws=P, ws_bytes=BIG):
    return N.lib().wsae_sta_update(P, P, k, hidden, None, n_rows, P, N.DT_F32, channels, channels, lags[0], lags[1], 0, f_cols,
                                   N.STA_TRIGGER_ALL, N.STA_WEIGHT_VALUE, P, P, P, ws, ws_bytes, None)


def runs_update(k=8, hidden=96, n_rows=0, n_seg=4, f_cols=96, ev_min_len=1, ws=P, ws_bytes=BIG):
    return N.lib().wsae_runs_update(P, P, k, hidden, P, n_rows, n_seg, 0, 0, f_cols, P, P, P, P, P, None, P, None, None, 0,
                                    ev_min_len, None, ws, ws_bytes, None)


def pool_update(k=8, hidden=96, n_rows=0, n_seg=4, f_cols=96, ld=96, ws=P, ws_bytes=BIG):
    return N.lib().wsae_pool_update(P, P, k, hidden, P, n_rows, n_seg, 0, f_cols, P, None, ld, P, ws, ws_bytes, None)


def sample_update(k=8, hidden=96, n_rows=0, ord_base=0, f_cols=96, keep=4, ws=P, ws_bytes=BIG):
    return N.lib().wsae_sample_update(P, P, k, hidden, None, n_rows, ord_base, 0, f_cols, None, 1, keep, 0, P, P, P, ws, ws_bytes,
                                      None)


def profile_update(k=8, hidden=96, n_rows=0, f_cols=96):
    return N.lib().wsae_profile_update(P, P, k, hidden, None, n_rows, 0, f_cols, P, P, P, P, P, P, P, None, 0, None)


def feature_topk_update(rows=0, width=8, H=96, keep=4, ws_bytes=BIG):
    return N.lib().wsae_feature_topk_update(P, P, rows, width, H, keep, 0, P, P, P, P, P, ws_bytes, None)


K = "need 1 <= k <= 128 (got 0)"
ROWS = "need 0 <= n_rows <= 2^31 - 1 (got -1)"
HIDDEN = "hidden must be positive (got 0)"
N_COLS = "need 1 <= n_cols <= hidden = 96 (got 97)"
NO_COL_OF = "without col_of the columns are the 96 features (got n_cols 50)"
LISTS = "cap 8 entries need t_row and t_val"
LAG = "need -1024 <= lag <= 1024 (got 2000)"
ALIGNED = "the workspace must be 8-byte aligned"

# (entry point, arguments that differ from a valid call, the text behind "<entry point>: "); recorded from the library
# before the checks moved into the shared macros
CASES = [
    # ---- wsae_probe_plan: the column code, the lists, the workspace and its alignment
    (probe_plan, dict(k=0), K),
    (probe_plan, dict(k=129), "need 1 <= k <= 128 (got 129)"),
    (probe_plan, dict(hidden=0), HIDDEN),
    (probe_plan, dict(n_rows=-1), ROWS),
    (probe_plan, dict(n_cols=97), N_COLS),
    (probe_plan, dict(n_cols=50), NO_COL_OF),
    (probe_plan, dict(t_row=None), LISTS),
    (probe_plan, dict(t_val=None), LISTS),
    (probe_plan, dict(cap=-1), "cap -1 entries need t_row and t_val"),
    (probe_plan, dict(ws_bytes=8), "workspace too small (8 < 1024)"),
    (probe_plan, dict(n_rows=10, ws=None), "workspace too small (0 < 1024)"),
    (probe_plan, dict(ws=P + 4), ALIGNED),
    (probe_plan, dict(k=0, t_row=None), K),                                   # two mistakes: the earlier check speaks
    (probe_plan, dict(n_cols=50, cap=-1), NO_COL_OF),
    (probe_plan, dict(t_row=None, ws_bytes=8), LISTS),
    (probe_plan, dict(ws_bytes=8, ws=P + 4), "workspace too small (8 < 1024)"),
    # ---- wsae_probe_forward: the column code and the lag
    (probe_forward, dict(k=0), K),
    (probe_forward, dict(hidden=0), HIDDEN),
    (probe_forward, dict(n_rows=2 ** 31), "need 0 <= n_rows <= 2^31 - 1 (got 2147483648)"),
    (probe_forward, dict(n_cols=0), "need 1 <= n_cols <= hidden = 96 (got 0)"),
    (probe_forward, dict(n_cols=50), NO_COL_OF),
    (probe_forward, dict(lag=2000), LAG),
    (probe_forward, dict(lag=-1025), "need -1024 <= lag <= 1024 (got -1025)"),
    (probe_forward, dict(k=0, lag=2000), K),
    (probe_forward, dict(C=0, lag=2000), "need 1 <= n_classes <= 1024 (got 0)"),  # the classes come before the lag
    (probe_forward, dict(lag=2000, ldw=2), LAG),                                   # ... and the lag before ldw
    # ---- wsae_probe_backward: the lists, the workspace and its alignment
    (probe_backward, dict(t_row=None), LISTS),
    (probe_backward, dict(cap=-1), "cap -1 entries need t_row and t_val"),
    (probe_backward, dict(ws_bytes=8), "workspace too small (8 < 3328)"),
    (probe_backward, dict(n_rows=10, ws=None), "workspace too small (0 < 3584)"),
    (probe_backward, dict(ws=P + 4), ALIGNED),
    (probe_backward, dict(C=0, t_row=None), "need 1 <= n_classes <= 1024 (got 0)"),
    (probe_backward, dict(t_row=None, lde=2), LISTS),
    (probe_backward, dict(t_row=None, ws_bytes=8), LISTS),
    (probe_backward, dict(ws_bytes=8, ws=P + 4), "workspace too small (8 < 3328)"),
    # ---- wsae_gram_update: the column code, the lists, the workspace and its alignment
    (gram_update, dict(k=0), K),
    (gram_update, dict(hidden=0), HIDDEN),
    (gram_update, dict(n_rows=-1), ROWS),
    (gram_update, dict(n_cols=97), N_COLS),
    (gram_update, dict(n_cols=50, p_rows=50), NO_COL_OF),
    (gram_update, dict(t_val=None), LISTS),
    (gram_update, dict(n_rows=10, ws_bytes=8), "workspace too small (8 < 1024)"),
    (gram_update, dict(n_rows=10, ws=None), "workspace too small (0 < 1024)"),
    (gram_update, dict(ws=P + 4), ALIGNED),
    (gram_update, dict(k=0, t_row=None), K),
    (gram_update, dict(t_row=None, p_rows=0), LISTS),                          # the lists come before the row window
    (gram_update, dict(n_rows=10, t_row=None, ws_bytes=8), LISTS),
    (gram_update, dict(n_rows=10, ws_bytes=8, ws=P + 4), "workspace too small (8 < 1024)"),
    # ---- wsae_regress_forward: the column code, the lag and the alignment (its size check is its own)
    (regress_forward, dict(k=0), K),
    (regress_forward, dict(hidden=0), HIDDEN),
    (regress_forward, dict(n_rows=-1), ROWS),
    (regress_forward, dict(n_cols=97), N_COLS),
    (regress_forward, dict(n_cols=50), NO_COL_OF),
    (regress_forward, dict(lag=2000), LAG),
    (regress_forward, dict(ws=P + 4), ALIGNED),
    (regress_forward, dict(k=0, lag=2000), K),
    (regress_forward, dict(C=0, lag=2000), "need 1 <= n_targets <= 1024 (got 0)"),
    (regress_forward, dict(lag=2000, ldw=2), LAG),
    (regress_forward, dict(n_rows=10, ws_bytes=8, ws=P + 4), "workspace too small (8 < 256)"),
    # ---- wsae_label_update, wsae_profile_update: hidden
    (label_update, dict(hidden=0), HIDDEN),
    (label_update, dict(k=0, hidden=0), K),
    (label_update, dict(hidden=0, n_rows=-1), HIDDEN),
    (profile_update, dict(hidden=0), HIDDEN),
    (profile_update, dict(k=0, hidden=0), K),
    (profile_update, dict(hidden=0, f_cols=0), HIDDEN),
    # ---- wsae_sta_update: hidden, the workspace and its alignment
    (sta_update, dict(hidden=0), HIDDEN),
    (sta_update, dict(ws_bytes=8), "workspace too small (8 < 2304)"),
    (sta_update, dict(n_rows=10, ws=None), "workspace too small (0 < 3328)"),
    (sta_update, dict(ws=P + 4), ALIGNED),
    (sta_update, dict(k=0, hidden=0), K),
    (sta_update, dict(hidden=0, channels=0), HIDDEN),
    (sta_update, dict(lags=(2, 1), ws_bytes=8), "need -1024 <= lag_lo <= lag_hi <= 1024 and at most 64 lags (got 2 .. 1)"),
    (sta_update, dict(ws_bytes=8, ws=P + 4), "workspace too small (8 < 2304)"),
    # ---- wsae_runs_update, wsae_pool_update: the workspace
    (runs_update, dict(ws_bytes=8), "workspace too small (8 < 32)"),
    (runs_update, dict(n_rows=10, ws=None), "workspace too small (0 < 32)"),
    (runs_update, dict(ev_min_len=0, ws_bytes=8), "ev_min_len must be at least 1 (got 0)"),
    (runs_update, dict(f_cols=97, ws_bytes=8), "the window [0, 0 + 97) is outside [0, 96)"),
    (pool_update, dict(ws_bytes=8), "workspace too small (8 < 32)"),
    (pool_update, dict(n_rows=10, ws=None), "workspace too small (0 < 32)"),
    (pool_update, dict(ld=95, ws_bytes=8), "ld 95 < f_cols 96"),
    (pool_update, dict(k=0, ws_bytes=8), K),
    # ---- wsae_sample_update: hidden and the workspace
    (sample_update, dict(hidden=0), HIDDEN),
    (sample_update, dict(ws_bytes=8), "workspace too small (8 < 1280)"),
    (sample_update, dict(n_rows=10, ws=None), "workspace too small (0 < 2240)"),
    (sample_update, dict(k=0, hidden=0), K),
    (sample_update, dict(hidden=0, n_rows=-1), HIDDEN),
    (sample_update, dict(ord_base=-1, ws_bytes=8), "the ordinals -1 + [0, 0) leave [0, 2^31)"),
    (sample_update, dict(keep=0, ws_bytes=8), "need 1 <= n_strata <= 16 and 1 <= keep <= 64 (got 1, 0)"),
    # ---- wsae_feature_topk_update: its offsets and cursors are int32, so a call takes at most 2^31 - 1 entries; the bound
    # comes before the workspace
    (feature_topk_update, dict(rows=2 ** 28), "at most 2^31 - 1 entries per call (got 268435456 rows of 8)"),
    (feature_topk_update, dict(rows=2 ** 28, ws_bytes=8), "at most 2^31 - 1 entries per call (got 268435456 rows of 8)"),
    (feature_topk_update, dict(rows=2 ** 28 - 1, ws_bytes=8), "workspace too small (8 < 17179870400)"),
    (feature_topk_update, dict(rows=2 ** 32, width=1, H=1), "at most 2^32 - 1 rows per call"),
]


@pytest.mark.parametrize("call,kwargs,text", CASES, ids=[f"{c.__name__}-{'-'.join(kw)}" for c, kw, _ in CASES])
def test_the_whole_message_of_a_rejected_call(call, kwargs, text):
    assert call(**kwargs) != 0
    assert N.last_error() == f"wsae_{call.__name__}: {text}"


def test_the_valid_calls_of_this_file_are_accepted():
    """The defaults are valid (and have no rows: nothing is launched), so every case above fails for its own reason."""
    for call in (probe_plan, probe_forward, probe_backward, gram_update, regress_forward, label_update, sta_update, runs_update,
                 pool_update, sample_update, profile_update, feature_topk_update):
        assert call() == 0, (call.__name__, N.last_error())


def test_workspace_queries_reject_with_minus_one():
    """The four queries behind the shared column-code predicate, and the lag of the two forward ones."""
    lib = N.lib()
    queries = {"wsae_probe_plan_workspace_bytes": (), "wsae_probe_forward_workspace_bytes": (3, 0),
               "wsae_gram_workspace_bytes": (96, 80), "wsae_regress_forward_workspace_bytes": (3, 0)}
    for name, rest in queries.items():
        query = getattr(lib, name)
        assert query(10, 8, 96, 96, *rest) >= 0, name
        for bad in ((-1, 8, 96, 96), (2 ** 31, 8, 96, 96), (10, 0, 96, 96), (10, N.PROBE_MAX_K + 1, 96, 96), (10, 8, 0, 1),
                    (10, 8, 96, 0), (10, 8, 96, 97)):
            assert query(*bad, *rest) == -1, (name, bad)
        assert query(2 ** 31 - 1, N.PROBE_MAX_K, 96, 1, *((1, 80) if name == "wsae_gram_workspace_bytes" else rest)) >= 0, name
    for name in ("wsae_probe_forward_workspace_bytes", "wsae_regress_forward_workspace_bytes"):
        query = getattr(lib, name)
        for lag in (-1025, 1025):
            assert query(10, 8, 96, 96, 3, lag) == -1, (name, lag)
        for lag in (-1024, 1024):
            assert query(10, 8, 96, 96, 3, lag) >= 0, (name, lag)


def test_feature_topk_workspace_query_rejects_more_entries_than_int32():
    lib = N.lib()
    assert lib.wsae_feature_topk_workspace_bytes(2 ** 31, 96) == -1
    assert lib.wsae_feature_topk_workspace_bytes(2 ** 31 - 1, 96) == 1280 + 8 * (2 ** 31 - 1)
    assert lib.wsae_feature_topk_workspace_bytes(-1, 96) == -1 and lib.wsae_feature_topk_workspace_bytes(8, 0) == -1


SIZE_ROWS = (0, 1, 63, 64, 65, 65536, 70000)
# (query, [(the arguments behind n_rows, the bytes for every n_rows of SIZE_ROWS)]); wsae_feature_topk_workspace_bytes takes
# entries, not rows: (width, H), asked for n_rows * width entries.  Recorded from the library before the chunking of the rows
# and the head of the list workspace moved into csrc/wsae_lists.h: a layout that moves by a byte shows here.
SIZES = [
    ("wsae_sta_workspace_bytes", [
        ((1, 96, 0, 96), [2304, 2816, 2816, 2816, 3584, 919296, 951808]),
        ((1, 5000, 3, 4097), [82944, 83456, 83456, 83456, 100352, 17371904, 17260288]),
        ((1, 40960, 8192, 4096), [81920, 82432, 82432, 82432, 99328, 17367040, 17255424]),
        ((32, 96, 0, 96), [2304, 2816, 18688, 18688, 19456, 17172224, 18311680]),
        ((32, 5000, 3, 4097), [82944, 83456, 99328, 99328, 116224, 33624832, 34620160]),
        ((32, 40960, 8192, 4096), [81920, 82432, 98304, 98304, 115200, 33619968, 34615296]),
        ((128, 96, 0, 96), [2304, 3328, 66816, 67840, 69120, 67503872, 72071680]),
        ((128, 5000, 3, 4097), [82944, 83968, 147456, 148480, 165888, 83956480, 88380160]),
        ((128, 40960, 8192, 4096), [81920, 82944, 146432, 147456, 164864, 83951616, 88375296]),
    ]),
    ("wsae_probe_plan_workspace_bytes", [
        ((8, 1, 1), [512, 512, 512, 512, 512, 4352, 4352]),
        ((8, 96, 96), [1024, 1024, 1024, 1024, 1280, 393728, 390400]),
        ((8, 4097, 4097), [33280, 33280, 33280, 33280, 49664, 16797952, 16650496]),
        ((8, 8194, 4097), [33280, 33280, 33280, 33280, 49664, 16797952, 16650496]),
        ((128, 1, 1), [512, 512, 512, 512, 512, 4352, 4352]),
        ((128, 96, 96), [1024, 1024, 1024, 1024, 1280, 393728, 390400]),
        ((128, 4097, 4097), [33280, 33280, 33280, 33280, 49664, 16797952, 16650496]),
        ((128, 8194, 4097), [33280, 33280, 33280, 33280, 49664, 16797952, 16650496]),
    ]),
    ("wsae_probe_backward_workspace_bytes", [
        ((1, 1, 0), [512, 768, 768, 768, 768, 768, 1024]),
        ((1, 1, 2047), [512, 768, 768, 768, 768, 768, 1024]),
        ((1, 1, 2048), [512, 768, 768, 768, 768, 768, 1024]),
        ((1, 1, 100000), [768, 1024, 1024, 1024, 1024, 1024, 1280]),
        ((1, 3, 0), [512, 768, 768, 768, 768, 1280, 1536]),
        ((1, 3, 2047), [512, 768, 768, 768, 768, 1280, 1536]),
        ((1, 3, 2048), [512, 768, 768, 768, 768, 1280, 1536]),
        ((1, 3, 100000), [1536, 1792, 1792, 1792, 1792, 2304, 2560]),
        ((1, 70, 0), [1024, 1792, 1792, 1792, 1792, 18944, 20736]),
        ((1, 70, 2047), [1024, 1792, 1792, 1792, 1792, 18944, 20736]),
        ((1, 70, 2048), [1536, 2304, 2304, 2304, 2304, 19456, 21248]),
        ((1, 70, 100000), [27904, 28672, 28672, 28672, 28672, 45824, 47616]),
        ((63, 1, 0), [1024, 1280, 1280, 1280, 1280, 1280, 1536]),
        ((63, 1, 2047), [1024, 1280, 1280, 1280, 1280, 1280, 1536]),
        ((63, 1, 2048), [1024, 1280, 1280, 1280, 1280, 1280, 1536]),
        ((63, 1, 100000), [1536, 1792, 1792, 1792, 1792, 1792, 2048]),
        ((63, 3, 0), [2048, 2304, 2304, 2304, 2304, 2816, 3072]),
        ((63, 3, 2047), [2048, 2304, 2304, 2304, 2304, 2816, 3072]),
        ((63, 3, 2048), [2048, 2304, 2304, 2304, 2304, 2816, 3072]),
        ((63, 3, 100000), [3328, 3584, 3584, 3584, 3584, 4096, 4352]),
        ((63, 70, 0), [35840, 36608, 36608, 36608, 36608, 53760, 55552]),
        ((63, 70, 2047), [35840, 36608, 36608, 36608, 36608, 53760, 55552]),
        ((63, 70, 2048), [36352, 37120, 37120, 37120, 37120, 54272, 56064]),
        ((63, 70, 100000), [62720, 63488, 63488, 63488, 63488, 80640, 82432]),
        ((4097, 1, 0), [66048, 66304, 66304, 66304, 66304, 66304, 66560]),
        ((4097, 1, 2047), [66048, 66304, 66304, 66304, 66304, 66304, 66560]),
        ((4097, 1, 2048), [66048, 66304, 66304, 66304, 66304, 66304, 66560]),
        ((4097, 1, 100000), [66304, 66560, 66560, 66560, 66560, 66560, 66816]),
        ((4097, 3, 0), [131584, 131840, 131840, 131840, 131840, 132352, 132608]),
        ((4097, 3, 2047), [131584, 131840, 131840, 131840, 131840, 132352, 132608]),
        ((4097, 3, 2048), [131584, 131840, 131840, 131840, 131840, 132352, 132608]),
        ((4097, 3, 100000), [132608, 132864, 132864, 132864, 132864, 133376, 133632]),
        ((4097, 70, 0), [2327552, 2328320, 2328320, 2328320, 2328320, 2345472, 2347264]),
        ((4097, 70, 2047), [2327552, 2328320, 2328320, 2328320, 2328320, 2345472, 2347264]),
        ((4097, 70, 2048), [2328064, 2328832, 2328832, 2328832, 2328832, 2345984, 2347776]),
        ((4097, 70, 100000), [2354432, 2355200, 2355200, 2355200, 2355200, 2372352, 2374144]),
    ]),
    ("wsae_sample_workspace_bytes", [
        ((8, 96, 0, 96, 1, 1), [1280, 1376, 7328, 7424, 7520, 6292736, 6721280]),
        ((8, 96, 0, 96, 1, 64), [1280, 1376, 7328, 7424, 7520, 6292736, 6721280]),
        ((8, 346, 2, 341, 3, 1), [12288, 12384, 18336, 18432, 18528, 6303744, 6732288]),
        ((8, 346, 2, 341, 3, 64), [12288, 12384, 18336, 18432, 18528, 6303744, 6732288]),
        ((8, 1030, 0, 1025, 1, 1), [12544, 12640, 18592, 18688, 18784, 6304000, 6732544]),
        ((8, 1030, 0, 1025, 1, 64), [12544, 12640, 18592, 18688, 18784, 6304000, 6732544]),
        ((8, 3072, 0, 3072, 16, 1), [590080, 590176, 596128, 596224, 596320, 6881536, 7310080]),
        ((8, 3072, 0, 3072, 16, 64), [590080, 590176, 596128, 596224, 596320, 6881536, 7310080]),
        ((128, 96, 0, 96, 1, 1), [1280, 2816, 98048, 99584, 101120, 100664576, 107521280]),
        ((128, 96, 0, 96, 1, 64), [1280, 2816, 98048, 99584, 101120, 100664576, 107521280]),
        ((128, 346, 2, 341, 3, 1), [12288, 13824, 109056, 110592, 112128, 100675584, 107532288]),
        ((128, 346, 2, 341, 3, 64), [12288, 13824, 109056, 110592, 112128, 100675584, 107532288]),
        ((128, 1030, 0, 1025, 1, 1), [12544, 14080, 109312, 110848, 112384, 100675840, 107532544]),
        ((128, 1030, 0, 1025, 1, 64), [12544, 14080, 109312, 110848, 112384, 100675840, 107532544]),
        ((128, 3072, 0, 3072, 16, 1), [590080, 591616, 686848, 688384, 689920, 101253376, 108110080]),
        ((128, 3072, 0, 3072, 16, 64), [590080, 591616, 686848, 688384, 689920, 101253376, 108110080]),
    ]),
    ("wsae_feature_topk_workspace_bytes", [
        ((1, 1), [256, 264, 760, 768, 776, 524544, 560256]),
        ((1, 63), [768, 776, 1272, 1280, 1288, 525056, 560768]),
        ((1, 64), [1024, 1032, 1528, 1536, 1544, 525312, 561024]),
        ((1, 1023), [12288, 12296, 12792, 12800, 12808, 536576, 572288]),
        ((1, 3072), [37120, 37128, 37624, 37632, 37640, 561408, 597120]),
        ((1, 40960), [491776, 491784, 492280, 492288, 492296, 1016064, 1051776]),
        ((32, 1), [256, 512, 16384, 16640, 16896, 16777472, 17920256]),
        ((32, 63), [768, 1024, 16896, 17152, 17408, 16777984, 17920768]),
        ((32, 64), [1024, 1280, 17152, 17408, 17664, 16778240, 17921024]),
        ((32, 1023), [12288, 12544, 28416, 28672, 28928, 16789504, 17932288]),
        ((32, 3072), [37120, 37376, 53248, 53504, 53760, 16814336, 17957120]),
        ((32, 40960), [491776, 492032, 507904, 508160, 508416, 17268992, 18411776]),
    ]),
]


@pytest.mark.parametrize("name,table", SIZES, ids=[name for name, _ in SIZES])
def test_workspace_sizes_are_pinned(name, table):
    query = getattr(N.lib(), name)
    for args, want in table:
        if name == "wsae_feature_topk_workspace_bytes":
            got = [query(rows * args[0], args[1]) for rows in SIZE_ROWS]
        else:
            got = [query(rows, *args) for rows in SIZE_ROWS]
        assert got == want, (name, args)
