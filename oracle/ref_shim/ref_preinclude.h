/*
 * TEST INFRASTRUCTURE ONLY — forced pre-include (-include) of the translation
 * unit that compiles the reference's headers (oracle/Makefile.ref).
 *
 * The reference takes sinf/cosf/tanf/powf and cos/sin from CUDA's libdevice,
 * which does not exist here; the project's kernels and oracle take them from
 * csrc/rt_libm.h.  A path branches on every float, so one ulp in one of these
 * moves whole pixels (DESIGN.md §3 records the count with glibc's functions).
 * This header therefore routes the reference's calls to rt_libm.h.  Every
 * standard header the reference includes is included first, so the macros
 * below meet only the reference's own text.
 */
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <list>
#include <map>
#include <math.h>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#ifndef REF_GLIBC_LIBM /* -DREF_GLIBC_LIBM: leave the host libm in place (the measurement in DESIGN.md §3) */
#include "rt_libm.h"

static inline float ref_shim_sin(float x) { return rt_sinf(x); }
static inline double ref_shim_sin(double x) { return rt_sin_d(x); }
static inline float ref_shim_cos(float x) { return rt_cosf(x); }
static inline double ref_shim_cos(double x) { return rt_cos_d(x); }

#define sinf rt_sinf
#define cosf rt_cosf
#define tanf rt_tanf
#define powf rt_powf
#define sin(x) ref_shim_sin(x)
#define cos(x) ref_shim_cos(x)
#endif
