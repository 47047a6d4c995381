// Sorted top-n list held in registers, shared by the selections whose order is "value descending, then index ascending"
// (wsae_match.hip, wsae_coact.hip).  The order is total, so what a list keeps never depends on who saw a candidate first.
#pragma once

constexpr int MT_EMPTY = 0x7fffffff;  // index of an unused list slot (value -inf); no real column reaches it

// (v, i) into the list sorted by value descending, then index ascending; the last element falls out.  All indexing
// is static: the list stays in registers.
template <int NB>
__device__ __forceinline__ void mt_insert(float (&lv)[NB], int (&li)[NB], float v, int i) {
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        const float tv = lv[p];
        const int ti = li[p];
        const bool b = v > tv || (v == tv && i < ti);
        lv[p] = b ? v : tv;
        li[p] = b ? i : ti;
        v = b ? tv : v;
        i = b ? ti : i;
    }
}
