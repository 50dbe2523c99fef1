// The vector-kernel files as one translation unit, so one code object, as vec_kernels.hip was: built as four code
// objects the same kernels cost the default bench.py line 0.6 %. Each file compiles alone too.
#include "reduce.hip"
#include "loss.hip"
#include "blas1.hip"
#include "hist.hip"
#include "adam.hip"
