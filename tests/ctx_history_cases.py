"""Case tables of tests/test_gpu_ctx_history.py: one ``wsae_ctx`` serving batches of several sizes, dtypes and intruding
calls.  Pure Python, importable without a GPU; tests/test_ctx_history_cases.py checks the tables against what they claim.

A *victim* is one training forward + backward.  Its *undisturbed* run happens on a fresh module whose ctx is created for
exactly that batch.  A *history* run does other work on the same module first (part A), or between the victim's forward
and its backward (part B); the products of the two runs must be bit-identical.  Sizes that depend on the device are
functions of ``cus``, the compute-unit count (256 on the MI355X).

``counts``: kernel launches on the kept ctx from the end of ``big`` to the end of the case (``wsae_profile_read`` names),
fixed by reading the dispatch code:

* every full forward is one ``encode_gemm`` and one ``decode`` launch (``wsae_encode_decode``, or ``wsae_encode_topk`` +
  ``wsae_decode_loss``); ``encode_compact``, ``encode``, ``pre_activation``, ``SAEIntervention.apply`` and
  ``SAEAttribution.attribute`` are one ``encode_gemm`` launch and no ``decode``;
* a backward whose forward is no longer the last call on the ctx restages: one more ``encode_gemm`` and one more ``decode``;
* ``stage_batch`` runs for every encoder launch except a bf16 batch in bf16 mode, which the GEMM gathers itself;
* ``bucket`` runs once per ``wsae_weight_grads`` unless the chunked decode sorted the code itself (``ent_valid``).
"""

from __future__ import annotations

from typing import NamedTuple, Optional

WSAE_MAX_PARTIALS = 1024
ANCHOR_MAX_B = 2320

# the host-side state of struct wsae_ctx (csrc/wsae_common.h) the cases are there for
FLAGS = ("xT_valid", "g_is_bf16", "g32_valid", "smax_valid", "pred_valid", "tmin_cur", "tmin", "ent_valid", "ent_vals",
         "ent_B", "wire_dec_vals", "n_dec_blocks", "n_sq_parts", "relu_x_B", "relu_g_B", "loss_cols", "relu_l1w", "btk_k",
         "btk_mode", "btk_state", "fired")

G12_DIMS = {"eq": (64, 64, 256, 8, 48), "narrow": (64, 32, 128, 8, 40)}  # tests/golden/g12_transcoders.npz


class Victim(NamedTuple):
    vid: str
    family: str          # topk | batchtopk | transcoder | skip | narrow | crosscoder | relu | relu_crosscoder
    prec: str            # arithmetic mode of the module
    x_dtype: str         # element type of the batch
    dims: tuple          # (D, H, k) as the constructor takes them; families with other shapes: see the rig
    B: int
    big: int             # the batch that sizes the ctx before the victim
    ragged: tuple        # tile sizes the row claims B is NOT a multiple of
    chunked: bool        # chunked MFMA decode (ceil(B / 64) >= cus): no CPU oracle, r14 / r18 / r19 hold the configuration
    dx: bool             # the input (and the target, where there is one) requires a gradient
    flow: Optional[str]  # ReLU SAE: "xgemm" (row-major-GEMM flow) or "general"
    there_for: str


def victims(cus: int) -> list:
    wide = (384, 3072, 32)
    ch = 64 * cus
    return [
        Victim("V1", "topk", "bf16", "bf16", wide, 1500, 2048, (64, 128, 256), False, False, None,
               "128x128 GEMM (smax_valid = pred_valid = 0), topk_rows, MFMA 4-wave decode (g_is_bf16, n_dec_blocks), ragged "
               "wgrad2s chunk, bucket_sort; xT_valid = 0"),
        Victim("V2", "topk", "bf16", "bf16", wide, 2320, 4096, (64, 128, 256), False, False, None,
               "persistent GEMM + selective strip stores (smax_valid, pred_valid, tmin_cur and the tmin rotation), ragged last "
               "256-row tile; n_sq_parts through the trainer"),
        Victim("V3", "topk", "bf16", "bf16", wide, ch, ch + 40, (), True, False, None,
               "chunked decode leaves ent_valid / ent_vals / ent_B; presorted wgrad2s"),
        Victim("V4", "topk", "bf16", "bf16", wide, ch + 40, ch + 128, (64,), True, False, None,
               "chunked decode with a ragged last chunk: ent_valid, ent_B"),
        Victim("V5", "topk", "fp32", "fp32", wide, 1500, 2048, (64, 128, 256), False, True, None,
               "stage_batch (xT_valid = 1, xT padding), decode_fast<float> (g_is_bf16 = 0, g32_valid), wgrad2<float>, "
               "wsae_input_grad"),
        Victim("V6", "topk", "bf16", "bf16", (96, 1024, 16), 300, 1000, (64, 128), False, False, None,
               "VALU decode (g_is_bf16 = 0), bucket_kernel with g->gT and x->xT blocks (xT_valid = 0), wgrad_kernel"),
        Victim("V7", "batchtopk", "bf16", "bf16", wide, 1500, 2048, (64, 128, 256), False, False, None,
               "selection workspace, btk_k / btk_mode / btk_state arming, fired = 0"),
        Victim("V8", "transcoder", "bf16", "bf16", wide, 1500, 2048, (64, 128, 256), False, True, None,
               "target != input, g32_valid, wsae_last_residual_grad, loss_cols = output width"),
        Victim("V9s", "skip", "fp32", "fp32", G12_DIMS["eq"][:4], G12_DIMS["eq"][4], 4 * G12_DIMS["eq"][4], (), False, True,
               None, "skip path through dt (g32_valid, wsae_last_residual_grad)"),
        Victim("V9n", "narrow", "fp32", "fp32", G12_DIMS["narrow"][:4], G12_DIMS["narrow"][4], 4 * G12_DIMS["narrow"][4], (),
               False, True, None, "loss_cols < D"),
        Victim("V10", "crosscoder", "fp32", "fp32", (24, 3, 128, 8), 50, 200, (), False, False, None,
               "padded engine width 96, loss_cols = d_model"),
        Victim("V11x", "relu", "bf16", "bf16", (128, 256), 256, 520, (), False, False, "xgemm",
               "relu_x_B, relu_g_B, relu_ws after the general flow; n_sq_parts through the trainer"),
        Victim("V11g", "relu", "bf16", "bf16", (128, 256), 200, 512, (64, 128), False, False, "general",
               "relu_x_B = relu_g_B = 0 after the row-major-GEMM flow, relu_ws, xT_valid"),
        Victim("V12", "relu_crosscoder", "bf16", "bf16", (64, 4, 512), 256, 512, (), False, False, None,
               "relu_l1w and loss_cols set and handed back"),
    ]


def victim(cus: int, vid: str) -> Victim:
    return next(v for v in victims(cus) if v.vid == vid)


CAUSAL_ROWS = 200
SPARSE = ("topk", "batchtopk", "transcoder", "skip", "narrow", "crosscoder")
DIRECT = ("topk", "batchtopk")  # families whose launch counts the tables carry (TopKSAE's own dispatch)


class Case(NamedTuple):
    cid: str
    vid: str
    kind: str            # part A: the history; part B: the intruder
    ctx: str             # "kept": one handle from before the history to after the victim; "replaced": it must differ
    batches: tuple       # every batch size that goes through the ctx before the victim's (last) call, ``big`` first
    counts: Optional[dict]
    there_for: str


def _stage(v: Victim, n_same_dtype: int, n_other_dtype: int) -> int:
    """``stage_batch`` launches of n encoder launches in the victim's dtype and n in the other one."""
    direct = v.prec == "bf16"  # bf16 mode: a bf16 batch is gathered by the GEMM, an fp32 batch is staged
    if direct:
        return n_other_dtype if v.x_dtype == "bf16" else n_same_dtype
    return n_same_dtype + n_other_dtype  # fp32 mode stages everything


def history_cases(cus: int) -> list:
    """Part A.  Every victim gets ``big`` and ``same``; V2, V3, V4, V5, V7 and V11 all that apply."""
    out = []
    full = ("V2", "V3", "V4", "V5", "V7", "V11x", "V11g")
    for v in victims(cus):
        kinds = ["big", "same"]
        if v.vid in full:
            kinds += ["dtype", "pending"]
            if v.family in ("topk", "batchtopk"):
                kinds.append("causal")
            kinds.append("params")
        for kind in kinds:
            batches = {"big": (v.big,), "causal": (v.big, CAUSAL_ROWS, CAUSAL_ROWS)}.get(kind, (v.big, v.B))
            counts = None
            if v.family in DIRECT and kind in ("big", "same", "dtype", "pending"):
                fwd = 1 if kind == "big" else 2
                wgrads = 2 if kind == "dtype" else 1
                counts = {"encode_gemm": fwd, "decode": fwd,
                          "stage_batch": _stage(v, fwd - (kind == "dtype"), int(kind == "dtype")),
                          "bucket": 0 if v.chunked else wgrads, "wgrad": wgrads}
            why = {"big": "the cap is larger than the batch: padding written by the kernels, not by creation-time zeros",
                   "same": "the no-backward decode instantiation at the victim's own sizes first",
                   "dtype": "xT_valid flips between the history and the victim",
                   "pending": "a forward whose backward never runs" + (": ent_valid = 1 for a dead buffer" if v.chunked else ""),
                   "causal": "SAEIntervention.apply and SAEAttribution.attribute on the ctx first",
                   "params": "parameters rewritten on the ctx: bf16 shadows, folded bias, _fresh / mark_fresh / invalidate"}[kind]
            out.append(Case(f"A-{v.vid}-{kind}", v.vid, kind, "kept", batches, counts, f"{why}; {v.there_for}"))
    return out


INTRUDERS = {
    "topk": ("nograd_same", "encode_small", "pre_activation", "intervention", "attribution", "second_ab", "second_ba", "over_cap"),
    "topk_short": ("nograd_same", "encode_small", "second_ab", "second_ba", "over_cap"),
    "batchtopk": ("nograd_same", "encode_small", "pre_activation", "intervention", "attribution", "second_ab", "second_ba",
                  "over_cap"),
    "sparse": ("nograd_same", "encode_small", "second_ab", "second_ba", "over_cap"),
    "relu": ("nograd_same", "second_ab", "second_ba", "over_cap"),
}
B_VICTIMS = {"V2": "topk", "V3": "topk_short", "V5": "topk", "V6": "topk_short", "V7": "batchtopk", "V8": "sparse", "V9s": "sparse",
             "V10": "sparse", "V11x": "relu", "V11g": "relu", "V12": "relu"}
# (encode_gemm, decode) launches between the end of ``big`` and the end of the victim's backward: the victim's forward, the
# intruder, the restage; ``second_ab``: both backwards restage, ``second_ba``: only the victim's
B_COUNTS = {"nograd_same": (3, 3), "encode_small": (3, 2), "pre_activation": (3, 2), "intervention": (3, 2),
            "attribution": (3, 2), "second_ab": (4, 4), "second_ba": (3, 3)}


def small(v: Victim) -> int:
    """The batch of ``encode_small`` / ``pre_activation``: smaller than the victim's and ragged."""
    return max(1, v.B // 2 - 3)


def over_cap(v: Victim) -> int:
    return v.big + 64


def intruder_cases(cus: int) -> list:
    """Part B: victim forward (grad mode), intruder, victim backward, on a ctx sized by ``big``."""
    out = []
    for v in victims(cus):
        if v.vid not in B_VICTIMS:
            continue
        for kind in INTRUDERS[B_VICTIMS[v.vid]]:
            if kind == "over_cap":
                nb, ctx = over_cap(v), "replaced"
            elif kind in ("encode_small", "pre_activation"):
                nb, ctx = small(v), "kept"
            elif kind in ("intervention", "attribution"):
                nb, ctx = CAUSAL_ROWS, "kept"
            else:
                nb, ctx = v.B, "kept"
            counts = None
            if ctx == "kept" and v.family in SPARSE:
                counts = dict(zip(("encode_gemm", "decode"), B_COUNTS[kind]))
            why = ("the ctx is destroyed and recreated: nobody's staged batch" if ctx == "replaced" else
                   "the restage protocol (SAEEngine.generation): xT / g / gT / dpre rebuilt for the victim")
            out.append(Case(f"B-{v.vid}-{kind}", v.vid, kind, ctx, (v.big, v.B, nb), counts, f"{why}; {v.there_for}"))
    return out


# Part C: SAETrainer.train_step over an epoch with a ragged last-but-one batch, on one ctx and on a fresh ctx per step
EPOCHS = [
    ("C-topk-bf16", "topk", "bf16", (384, 3072, 32), (2048, 2048, 1500, 2048), "n_sq_parts, tmin rotation across steps, fired = 0"),
    ("C-topk-fp32", "topk", "fp32", (384, 3072, 32), (2048, 2048, 1500, 2048), "n_sq_parts, xT_valid, smax_valid on fp32 pre"),
    ("C-batchtopk-bf16", "batchtopk", "bf16", (384, 3072, 32), (2048, 2048, 1500, 2048), "btk_k, btk_mode, btk_state per step"),
    ("C-relu-bf16", "relu", "bf16", (128, 256), (512, 512, 200, 512), "relu_x_B, relu_g_B, n_sq_parts, relu_ws per ctx"),
]

# Part D: the control - without the restage the backward reads the intruder's staged state
CONTROLS = [
    ("D-V2", "V2", "wsae_weight_grads after a grad-mode forward of other rows at the same B: g_is_bf16 / gb and the bucketed "
                   "code are the intruder's; wire_dec_vals stays null (one launch for both matrices)"),
    ("D-V11x", "V11x", "wsae_relu_backward after a forward of other rows at the same B: relu_x_B == relu_g_B == B, the bf16 "
                       "hidden, the activity bits and g are the intruder's"),
]


def all_there_for(cus: int) -> list:
    return ([c.there_for for c in history_cases(cus)] + [c.there_for for c in intruder_cases(cus)] +
            [e[5] for e in EPOCHS] + [c[2] for c in CONTROLS])
