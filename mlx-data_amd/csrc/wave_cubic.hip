// wave_cubic.hip -- the scatter wave kernels of the cubic filters
// (Catmull-Rom, Mitchell, B-spline: S = 4 accumulator slots; wave.hip
// select_scatter under MXD_WAVE_CUBIC_TU lists the shapes) as a translation
// unit of their own, compiled beside wave.o.  The kernel source is wave.hip's.
#define MXD_WAVE_CUBIC_TU 1
#include "wave.hip"
