// ka_kmeans.h -- library-internal: the 2-means bisection of build_tree_kmeans on the device (ka_kmeans.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

struct KaKmNode {
        int left = -1, right = -1;           // indices into the node vector; left < 0: a leaf cluster
        std::vector<int> cluster;            // its members in the reference's order
};

// dm: numseq x 32 floats (host), 32 anchors.  nodes[0] is the root.  Returns 0, or 1 with `err` set.
int ka_kmeans_device(int device, hipStream_t stream, const float* dm, int numseq, std::vector<KaKmNode>& nodes, std::string& err);

// Tests only (ka_debug_kmeans_level, include/kalign_amd.h): one level exactly as ka_kmeans_device runs it, every candidate's
// results handed back.  Returns 0, or 1 with `err` set.
int ka_kmeans_debug_level(int device, hipStream_t stream, const float* dm, int numrows, const int* samples, int n_samples,
                          const int* sets_start_n, int n_sets, int force_big,
                          float* score, int* counts, int* lists, float* mind, float* wmean, int* winner, int* big_out, std::string& err);
