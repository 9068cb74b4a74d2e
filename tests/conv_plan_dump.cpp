// conv_plan_dump — prints the conv dispatch plans of the cases on stdin, one
// JSON object per case (tests/test_conv_plan.py).  Host code only: it calls
// the planners of libtensorium_hip.so, creates no context and makes no HIP call.
//
//   fwd ID batch C H W filters k stride pad dil act fused bias_act w_aligned [opt=value]...
//   bwd ID batch C H W filters k stride pad dil act has_bn has_state_delta d_aligned [opt=value]...
//
// opt is a field of tns::Options; every other field keeps its default.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../tensorium_amd/csrc/tns_internal.hpp"
#include "../tensorium_amd/csrc/tns_ctx.hpp"

using namespace tns;

static bool set_opt(Options& o, const std::string& kv) {
  const size_t eq = kv.find('=');
  if (eq == std::string::npos) return false;
  const std::string k = kv.substr(0, eq);
  const long long v = atoll(kv.c_str() + eq + 1);
  struct { const char* name; int64_t* p; } f[] = {
      {"strict_beta0", &o.strict_beta0}, {"nt_sdot", &o.nt_sdot}, {"dx_fused", &o.dx_fused},
      {"dx_tile", &o.dx_tile}, {"dx_conv", &o.dx_conv}, {"dw_res", &o.dw_res},
      {"dw_tile", &o.dw_tile}, {"bwd_overlap", &o.bwd_overlap}, {"derive_sums", &o.derive_sums},
      {"scratch_cap", &o.scratch_cap}, {"tt_exact", &o.tt_exact}, {"srss_quirk", &o.srss_quirk},
      {"conv_variant", &o.conv_variant}, {"conv_pad", &o.conv_pad}};
  for (auto& e : f)
    if (k == e.name) {
      *e.p = v;
      return true;
    }
  if (k == "dx_c1") return o.dx_c1 = v != 0, true;
  if (k == "bn_fused") return o.bn_fused = v != 0, true;
  return false;
}

static std::string quoted(const char* s) {
  std::string r = "\"";
  for (; *s; ++s) {
    if (*s == '"' || *s == '\\') r += '\\';
    r += *s;
  }
  return r + "\"";
}

static void dump_dw(const char* key, const ConvDwChoice& d) {
  static const char* kDw[] = {"res", "tile", "sdot", "gemm"};
  printf(", \"%s\": {\"path\": \"%s\", \"form\": %d, \"col\": %s, \"part_elems\": %lld}", key,
         kDw[d.path], d.form, d.col ? "true" : "false", (long long)d.part_elems);
}

int main() {
  static const char* kFwd[] = {"empty", "unfused", "im2col", "direct", "conv1x1", "slab", "tile",
                               "implicit"};
  static const char* kDx[] = {"none", "conv1x1", "fused", "conv3", "conv3s2", "tile", "tn"};
  static const char* kSched[] = {"sequential", "joined", "pipelined"};
  auto tf = [](bool b) { return b ? "true" : "false"; };
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, id, kv;
    long long v[10];
    int a = 0, b = 0, al = 0;
    if (!(in >> kind >> id)) continue;
    for (auto& x : v) in >> x;
    in >> a >> b >> al;
    if (!in || (kind != "fwd" && kind != "bwd")) {
      fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    Options o;  // the defaults, then the case's forced options
    while (in >> kv)
      if (!set_opt(o, kv)) {
        fprintf(stderr, "bad option: %s\n", kv.c_str());
        return 2;
      }
    const ConvShape s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], (int32_t)v[9],
                      kind == "fwd" && al != 0};
    printf("{\"id\": %s, \"kind\": \"%s\"", quoted(id.c_str()).c_str(), kind.c_str());
    if (kind == "fwd") {
      const ConvFwdPlan p = plan_conv_forward(s, a, b != 0, o);
      printf(", \"err\": %d, \"msg\": %s, \"path\": \"%s\", \"form\": %d, \"implicit\": %s, "
             "\"epi_act\": %d, \"act_tail\": %s, \"needs_col\": %s, \"padded\": %s, "
             "\"chunk\": %lld, \"col_elems\": %lld, \"stage1_elems\": %lld}\n",
             p.err, quoted(p.msg).c_str(), kFwd[p.path], p.form, tf(p.implicit), p.epi_act,
             tf(p.act_tail), tf(p.needs_col), tf(p.padded), (long long)p.chunk,
             (long long)p.col_elems, (long long)p.stage1_elems);
    } else {
      const ConvBwdPlan p = plan_conv_backward(s, a != 0, b != 0, al != 0, o);
      printf(", \"err\": %d, \"msg\": %s, \"empty\": %s, \"bn_fused\": %s, \"derive_sums\": %s",
             p.err, quoted(p.msg).c_str(), tf(p.empty), tf(p.bn_fused), tf(p.derive_sums));
      dump_dw("dw", p.dw);
      dump_dw("dw_fallback", p.dw_fallback);
      printf(", \"dw_res_forced\": %s, \"dx\": \"%s\", \"dx_form\": %d, \"dx_tile\": %d, "
             "\"dx_tile_forced\": %s, \"dx_direct\": %s, \"needs_col\": %s, \"dx_col\": %s, "
             "\"sched\": \"%s\", \"bn_elems\": %lld, \"res_a_elems\": %lld, "
             "\"res_b_elems\": %lld, \"col_elems\": %lld, \"wt_elems\": %lld}\n",
             tf(p.dw_res_forced), kDx[p.dx], p.dx_form, p.dx_tile, tf(p.dx_tile_forced),
             tf(p.dx_direct), tf(p.needs_col), tf(p.dx_col), kSched[p.sched],
             (long long)p.bn_elems, (long long)p.res_a_elems, (long long)p.res_b_elems,
             (long long)p.col_elems, (long long)p.wt_elems);
    }
  }
  return 0;
}
