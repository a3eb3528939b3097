// Register vector types and the out-of-range buffer offset shared by every convolution file (conv_*.hip).
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define C2M_OOB 0x80000000u   // voffset beyond any tensor we accept (< 2 GiB): the buffer load returns 0, the buffer store is dropped
