// gemm_plan_dump — prints the GEMM dispatch plans of the cases on stdin, one
// JSON object per case (tests/test_gemm_plan.py).  Host code only: it calls
// tns_gemm_plan of libtensorium_hip.so, creates no context and makes no HIP
// call.
//
//   ID variant transA transB M N K lda ldb ldc strideA strideB strideC batch
//      alpha_is_one beta_mode epi a_aligned16 b_aligned16 nt_sdot tt_exact sdot_form
//
// (the TNS_GP_* order of include/tns.h).  A case tns_gemm_plan rejects prints
// {"id": ID, "rejected": the error message}.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../include/tns.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string id;
    long long variant = 0;
    int64_t v[TNS_GP_COUNT];
    if (!(in >> id)) continue;
    in >> variant;
    for (auto& x : v) {
      long long t = 0;
      in >> t;
      x = t;
    }
    if (!in) {
      fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    char buf[1024];
    if (tns_gemm_plan((int32_t)variant, v, buf, sizeof buf) != TNS_OK) {
      printf("{\"id\": \"%s\", \"rejected\": \"%s\"}\n", id.c_str(), tns_last_error());
      tns_clear_error();
      continue;
    }
    printf("{\"id\": \"%s\", %s\n", id.c_str(), buf + 1);
  }
  return 0;
}
