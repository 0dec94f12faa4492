// wide_bvh_caps.h — the list capacities of wf_long's wave-wide s_min query (wide_bvh.h), shared with its
// host restatement (host/wide_smin_host.h) and the CPU check that the shipped capacities do not overflow.
#pragma once
// (4 B per item of either list: 2 * 192 * 4 + 2 * 320 * 4 = 4,096 B, wf_long's per-wave frontier storage.  Sized on
// the 2M-triangle room: rays skimming a finely tessellated wall 1e-4 off its plane meet up to 281 leaf boxes and
// 157 inner ones in one round — tests/native/wide_smin_check.cpp's grazing rays; a deep path's chords stay below 60.)
#ifndef WSM_FCAP
#define WSM_FCAP 192 // frontier items per wave (two arrays: this round's, the next one's)
#endif
#ifndef WSM_LCAP
#define WSM_LCAP 320 // hit leaves per round (two arrays)
#endif
