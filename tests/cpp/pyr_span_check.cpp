// Prints the eager span of a pyramid level (orb_slam2_comment_amd/csrc/pyr_span.h, the sizing rule of the pyramid
// kernels' tables) for test_pyramid_span_cpu.py: argv = F edge pad_l rows_per_unit (w h)...; one line per level:
// col0 words row0 rows units
#include "pyr_span.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 7 || (argc - 5) % 2) return 2;
    const int F = atoi(argv[1]), edge = atoi(argv[2]), pad_l = atoi(argv[3]), rpu = atoi(argv[4]);
    for (int i = 5; i + 1 < argc; i += 2) {
        const orbhip::PyrSpan S = orbhip::pyr_span(atoi(argv[i]), atoi(argv[i + 1]), F, edge, pad_l);
        printf("%d %d %d %d %d\n", S.col0, S.words, S.row0, S.rows, orbhip::pyr_span_units(S, rpu));
    }
    return 0;
}
