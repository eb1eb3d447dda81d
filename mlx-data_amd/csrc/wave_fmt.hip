// wave_fmt.hip -- the formatted-output instantiations of wave.hip's kernels
// (output mode kOutFmt: resample_wave_fmt, one per shape wave.hip has in its
// u8 and f32 modes) and their launch, as a translation unit of their own so
// the build compiles them beside wave.o.  The kernel source is wave.hip's.
#define MXD_WAVE_FMT_TU 1
#include "wave.hip"
