// Host build of the library's own sincos_body (csrc/shipsim_internal.h), for tests/test_sincos.py: f64 arguments on stdin, (sin, cos)
// pairs on stdout, both as raw little-endian doubles.  Compiled as HIP source for the host alone, with -ffp-contract=off like the
// library: the routine is IEEE f64 arithmetic with fma and rint only, so these are the bits the device computes.
#include <cstdio>

#include "shipsim_internal.h"

int main()
{
    double a;
    while (fread(&a, sizeof a, 1, stdin) == 1) {
        double o[2];
        ssg::sincos_body(a, &o[0], &o[1]);
        if (fwrite(o, sizeof(double), 2, stdout) != 2) return 1;
    }
    return 0;
}
