// Which part of a padded pyramid plane the table-driven pyramid kernels write for a level >= 1 (no other header needed:
// tests/cpp/pyr_span_check.cpp compiles this file alone).
//
// A plane is prows = h + 2*edge rows of `pitch` bytes; level pixel (x, y) is byte pad_l + x of padded row edge + y.  An
// extraction writes the interior plus an eager frame of depth F <= edge around it: columns x in [-F, w + F), padded
// rows [edge - F, edge + h + F).  The rest of the REFLECT_101 frame is written on demand (ensure_frames).  The kernels
// store whole dwords, so the span starts at dword col0 of a row (4-byte aligned in the plane: pitch and pad_l are
// multiples of 4) and its last dword may carry up to 3 bytes right of the span, written as 0 like every byte outside
// the frame.  F = edge is the full frame as it was before there was a choice: from dword 0 of the row, which also
// zeroes the pad_l - edge bytes left of the frame.
#pragma once

namespace orbhip {
struct PyrSpan {
    int col0, words;   // first destination dword of a row, dwords per row
    int row0, rows;    // first padded row, rows
};
inline PyrSpan pyr_span(int w, int h, int F, int edge, int pad_l)
{
    PyrSpan S;
    if (F > edge) F = edge;
    if (F < 0) F = 0;
    S.col0 = F == edge ? 0 : (pad_l - F) >> 2;
    S.words = ((pad_l + w + F + 3) >> 2) - S.col0;
    S.row0 = edge - F;
    S.rows = h + 2 * F;
    return S;
}
// wavefront work items of a level: row groups x runs of <= 64 dwords (the rule of pyr_chunks)
inline int pyr_span_units(const PyrSpan &S, int rows_per_unit)
{
    return ((S.rows + rows_per_unit - 1) / rows_per_unit) * ((S.words + 63) / 64);
}
}   // namespace orbhip
