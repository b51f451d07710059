// tests/test_recurrent_row_plan_host.py: the pure rules of the recurrent row, compiled with g++ (no HIP header).
#include "sf_attention_plan.h"

extern "C" {
int shim_hh_accepts(int mt, int cpw) { return sf::pair_proj_score_hh_accepts(sf::SmallInst{mt, cpw}) ? 1 : 0; }
int shim_recurrent_row_cell(int K_x, int H) { return sf::recurrent_row_cell(K_x, H) ? 1 : 0; }
int shim_small_shape(int M, int N, int chunks, int* mt, int* cpw) {
    return sf::plan_detail::small_shape(M, N, chunks, mt, cpw) ? 1 : 0;
}
}
