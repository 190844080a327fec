// The f64 reduction tree of csrc/ccx_tree.h compiled for the host BY ITSELF (tests/test_tree_host.py: -O2 -ffp-contract=off),
// behind a C interface for ctypes.  Nothing but that header is included, and there is no arithmetic here.
#include "ccx_tree.h"

extern "C" {

double tree_sum_host(long long M, const double* terms) { return ccx_tree::sum_host(terms, M); }

double tree_block_host(int n, const double* terms) { return ccx_tree::block_host(terms, n); }

double tree_final_host(long long B, const double* partials) { return ccx_tree::final_host(partials, B); }

long long tree_blocks_of(long long M) { return ccx_tree::blocks_of(M); }

}  // extern "C"
