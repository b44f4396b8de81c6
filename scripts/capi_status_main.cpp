// Replays the cases of tests/golden/capi_status_table.json against the launchers' objects in a stand-alone program, so that the host
// side of libpfk.so can run under the sanitizers (a library loaded into python cannot):
//
//   python scripts/capi_status_table.py --dump cases.txt
//   for f in ptlflow_amd/csrc/pfk_*.hip; do hipcc --offload-arch=gfx950 -O3 -g -std=c++17 -fPIC -fno-gpu-rdc -Iinclude -Iptlflow_amd/csrc \
//       -Xarch_host -fsanitize=address,undefined -c $f -o obj/$(basename $f .hip).o; done     (pfk_stamp.hip: -DPFK_SOURCE_HASH='"x"')
//   $ROCM_PATH/lib/llvm/bin/clang++ -std=c++17 -g -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude -fsanitize=address,undefined \
//       -c scripts/capi_status_main.cpp -o obj/main.o                                         (host C++: hipcc would take it for HIP)
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined obj/*.o -o capi_status_main && ./capi_status_main cases.txt
//
// A line is `entry expected descriptor-bytes-in-hex argument ...` (scripts/capi_status_table.py::dump).  ONLY without a GPU: the
// descriptors sit on made-up addresses, and an accepted one answers PFK_ERR_LAUNCH because there is no device to launch on.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pfk.h"

namespace {

struct Args {
  std::vector<std::string> tok;
  size_t next = 0;
  int host[3];
  long long ll() { return std::stoll(tok.at(next++)); }
  int i() { return (int)ll(); }
  float f() { return std::stof(tok.at(next++)); }
  template <class T = void>
  T* p() { return reinterpret_cast<T*>((uintptr_t)std::stoull(tok.at(next++))); }
  const int* ints() {      // h:a,b,c or h:null
    const std::string t = tok.at(next++).substr(2);
    if (t == "null") return nullptr;
    if (sscanf(t.c_str(), "%d,%d,%d", &host[0], &host[1], &host[2]) != 3) abort();
    return host;
  }
};

char letter(long long r, bool query) {
  static const char L[] = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";
  if (query && r >= 0) return L[r % 52];
  return (r <= 0 && r >= -9) ? (char)('0' - r) : '?';
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) { fprintf(stderr, "a GPU is visible: not replaying made-up addresses\n"); return 2; }
  (void)hipGetLastError();
  std::ifstream in(argv[1]);
  std::string line;
  long long n = 0, bad = 0;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string name, want, hex, t;
    ss >> name >> want >> hex;
    Args a;
    while (ss >> t) a.tok.push_back(t);
    // the descriptor(s) in an exactly sized heap block: a read past the end is the sanitizer's to report
    std::vector<unsigned char> blob(hex.size() / 2);
    for (size_t k = 0; k < blob.size(); ++k) blob[k] = (unsigned char)std::stoi(hex.substr(2 * k, 2), nullptr, 16);
    const pfk_conv_desc* d = reinterpret_cast<const pfk_conv_desc*>(blob.data());
    const pfk_conv_b16_desc* e = reinterpret_cast<const pfk_conv_b16_desc*>(blob.data());
    long long r;
    bool query = false;
    if (name == "pfk_conv2d_f32") r = pfk_conv2d_f32(d, nullptr);
    else if (name == "pfk_conv2d_group_f32") r = pfk_conv2d_group_f32(d, a.i(), nullptr);
    else if (name == "pfk_conv2d_bf16s") { void* w = a.p(); r = pfk_conv2d_bf16s(d, w, a.i(), nullptr); }
    else if (name == "pfk_conv2d_b16") r = pfk_conv2d_b16(e, nullptr);
    else if (name == "pfk_conv2d_gelu_b16") r = pfk_conv2d_gelu_b16(e, nullptr);
    else if (name == "pfk_conv2d_wino_f32") r = pfk_conv2d_wino_f32(d, nullptr);
    else if (name == "pfk_conv2d_wino_res_f32") r = pfk_conv2d_wino_res_f32(d, nullptr);
    else if (name == "pfk_conv2d_wino_norm_f32") { float* m = a.p<float>(); float* s = a.p<float>(); r = pfk_conv2d_wino_norm_f32(d, m, s, a.i(), nullptr); }
    else if (name == "pfk_conv2d_wino_stats_f32") {
      float* m = a.p<float>(); float* s = a.p<float>(); const int relu = a.i(); const float eps = a.f();
      float* om = a.p<float>(); float* os = a.p<float>(); void* ws = a.p(); const long long wb = a.ll();
      r = pfk_conv2d_wino_stats_f32(d, m, s, relu, eps, om, os, ws, wb, nullptr);
    }
    else if (name == "pfk_conv1d_wino_f32") r = pfk_conv1d_wino_f32(d, nullptr);
    else if (name == "pfk_conv_wgrad_f32") {
      float* dy = a.p<float>(); const int ld = a.i(); float* dw = a.p<float>(); const int wb = a.i(); void* ws = a.p(); const long long wsb = a.ll();
      r = pfk_conv_wgrad_f32(d, dy, ld, dw, wb, ws, wsb, nullptr);
    }
    else if (name == "pfk_conv_wgrad_unpacked_f32" || name == "pfk_conv_wgrad_unpacked_b16") {
      const int* rc = a.ints(); void* dy = a.p(); const int ld = a.i(); const int cr = a.i(); float* dw = a.p<float>(); float* db = a.p<float>();
      const int acc = a.i(); void* ws = a.p(); const long long wsb = a.ll();
      r = name.back() == '2' ? pfk_conv_wgrad_unpacked_f32(d, rc, static_cast<const float*>(dy), ld, cr, dw, db, acc, ws, wsb, nullptr)
                             : pfk_conv_wgrad_unpacked_b16(e, rc, dy, ld, cr, dw, db, acc, ws, wsb, nullptr);
    }
    else {
      query = true;
      if (name == "pfk_conv_ktot") r = pfk_conv_ktot(d);
      else if (name == "pfk_conv_ktot_bf16") r = pfk_conv_ktot_bf16(d);
      else if (name == "pfk_conv_ktot_b16") r = pfk_conv_ktot_b16(e);
      else if (name == "pfk_conv_wgrad_workspace_bytes") r = pfk_conv_wgrad_workspace_bytes(d, a.i());
      else if (name == "pfk_conv_wgrad_unpacked_workspace_bytes") r = pfk_conv_wgrad_unpacked_workspace_bytes(d, a.i());
      else if (name == "pfk_conv_wgrad_unpacked_b16_workspace_bytes") r = pfk_conv_wgrad_unpacked_b16_workspace_bytes(e, a.i());
      else if (name == "pfk_conv_wino_weight_floats") { const int c = a.i(); r = pfk_conv_wino_weight_floats(c, a.i()); }
      else if (name == "pfk_conv_wino1d_weight_floats") { const int k = a.i(); r = pfk_conv_wino1d_weight_floats(k, a.i()); }
      else if (name == "pfk_conv_wino_stats_workspace_bytes") { const int B = a.i(), H = a.i(), W = a.i(); r = pfk_conv_wino_stats_workspace_bytes(B, H, W, a.i()); }
      else { fprintf(stderr, "unknown entry point %s\n", name.c_str()); return 2; }
    }
    ++n;
    if (letter(r, query) != want[0] && ++bad <= 10) fprintf(stderr, "case %lld %s: answers %lld, recorded '%s'\n", n, name.c_str(), r, want.c_str());
  }
  printf("%lld cases replayed, %lld differ from the recorded table\n", n, bad);
  return bad ? 1 : 0;
}
