// ka_forest.h -- the records the realignment-tree kernels (ka_rows.hip) and their host side (ka_api.cpp) share.  Library-internal.
#pragma once
#include <hip/hip_runtime.h>

// The realignment tree is built for a batch of families; one family is a batch of one (ka_aln_guide_tree).
// One UPGMA: an n x n matrix, a flag per row, two sets of row keys (the per-merge launches only), n - 1 merges.
struct KaUpgma { float* dm; int* active; unsigned long long* key[2]; int2* merges; int n; };

#define KA_UPGMA_NT 512                      // threads of the one-workgroup UPGMA
#define KA_UPGMA_ONE_WG_MAX 6144             // rows it takes (its LDS: 17 bytes per row); a larger family: one launch per merge
#define KA_UPGMA_CLASSES 5                   // its size classes: n <= 512, 1024, 2048, 4096, 6144 (1, 2, 4, 8, 12 rows per thread)
static inline int ka_upgma_class(int n) { return n <= KA_UPGMA_NT ? 0 : n <= 2 * KA_UPGMA_NT ? 1 : n <= 4 * KA_UPGMA_NT ? 2 : n <= 8 * KA_UPGMA_NT ? 3 : 4; }

// One KaAdTile per workgroup of the identity distances: tile (ti, tj), tj >= ti, of the family whose rows start at row0; n rows,
// alnlen columns of its own, its matrix at dm + dm_off.  One KaAdFam per family, for the row means.
struct KaAdTile { int row0, n, alnlen, ti, tj, pad; long long dm_off; };
struct KaAdFam { int first, n; long long dm_off; };
