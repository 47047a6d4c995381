"""The host-side argument checks that the analysis entry points share (``CW_REQUIRE_*`` in csrc/wsae_codewalk.h), seen
from outside and without a GPU: the WHOLE text of ``wsae_last_error()`` for every shared requirement of every entry point
that makes it, and, with two mistakes in one call, which of the two messages the caller gets - the order of the checks.
Host buffers stand in for the device pointers: a rejected call launches nothing and never follows them.  Apart from the
cases that leave the workspace pointer out, which a call with rows alone rejects, the calls have no rows, so that even an
accepted call would launch nothing."""

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
]


@pytest.mark.parametrize("call,kwargs,text", CASES, ids=[f"{c.__name__}-{'-'.join(kw)}" for c, kw, _ in CASES])
def test_the_whole_message_of_a_rejected_call(call, kwargs, text):
    assert call(**kwargs) != 0
    assert N.last_error() == f"wsae_{call.__name__}: {text}"


def test_the_valid_calls_of_this_file_are_accepted():
    """The defaults are valid (and have no rows: nothing is launched), so every case above fails for its own reason."""
    for call in (probe_plan, probe_forward, probe_backward, gram_update, regress_forward, label_update, sta_update, runs_update,
                 pool_update, sample_update, profile_update):
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
