// rsmp_hd.h -- RSMP_HD: the qualifiers of a function that compiles for the host and for the device.  No include: under
// hipcc the compiler itself knows the two words, a host compiler (the stand-alone tests) sees no qualifiers.
#pragma once

#if defined(__HIPCC__)
#define RSMP_HD __host__ __device__
#else
#define RSMP_HD
#endif
