// Host program behind tests/test_gemm_launch_cpu.py: what launch_gemm / launch_gemm_mx answer to a fixed list of argument
// sets on a machine WITHOUT a GPU, and the launch shape the library derives for the sets it accepts.
//
// Without a device an accepted launch ends in hipErrorInvalidDevice (101) where the launcher asks for the current
// device, after every argument check has run; a refused one ends in hipErrorInvalidValue (1).  The buffers are 64-byte
// dummies, so this must never run where a launch could succeed: with a device present it prints nothing and exits 77.
//
// Per case:   case <name>
//             [  shape <tiles_m> <tiles_n> <gn> <nt_store> <lds_bytes> <block> <persistent_wanted> <epilogue> <stats_off>]
//               rc <hipError_t>
// The shape line comes from build_gemm_launch / build_mx_launch (gemm_launch.h; -DVDR_CASES_NO_BUILDER: from a library
// that predates them and prints the line itself -- how tests/ledger/gemm_launch_cases.txt was recorded).  Compiled as HIP
// (gemm_launch.h holds the kernels' argument block), linked to libvdr.so.
#include <cstdio>
#include <cstring>

#ifdef VDR_CASES_NO_BUILDER
#include "vdr_kernels.h"
#else
#include "gemm_launch.h"
#endif

using namespace vdr;

alignas(64) static char g_buf[64];

static GemmArgs base(int64_t M, int N, int K) {
  GemmArgs a{};
  a.A = a.W = a.C = g_buf;
  a.bias = (const float*)g_buf;
  a.M = M;
  a.N = N;
  a.K = K;
  a.lda = a.ldw = K;
  a.ldc = a.ldr = N;
  a.omap = identity_map();
  return a;
}

static void run(const char* name, const GemmArgs& a, int epi, int variant, bool mx = false) {
  printf("case %s\n", name);
#ifndef VDR_CASES_NO_BUILDER
  GemmLaunch L;
  if ((mx ? build_mx_launch(a, epi, variant, &L) : build_gemm_launch(a, epi, variant, &L)) == hipSuccess && L.lds)  // (lds 0: variant 31)
    printf("  shape %d %d %d %d %zu %d %d %d %d\n", L.k.tiles_m, L.k.tiles_n, L.k.gn, L.k.nt_store, L.lds, L.row->block(), (int)L.persistent,
           L.epi, L.k.stats_off);
#endif
  const hipError_t e = mx ? launch_gemm_mx(a, epi, variant, nullptr) : launch_gemm(a, epi, variant, nullptr);
  printf("  rc %d\n", (int)e);
}

static char g_name[256];
#define NAME(...) (snprintf(g_name, sizeof g_name, __VA_ARGS__), g_name)

static GemmArgs resid(GemmArgs a) {
  a.resid = g_buf;
  return a;
}
static GemmArgs with_cpart(GemmArgs a, int groups) {
  a.ln_cpart = (const float*)g_buf;
  a.colsum = (const float*)g_buf;
  a.ln_groups = groups;
  a.ln_cstride = a.M;
  a.ln_eps = 1e-6f;
  return a;
}
static GemmArgs with_fin(GemmArgs a, bool cnt, bool part) {
  a.fin_stats = (float*)g_buf;
  a.fin_cnt = cnt ? (uint32_t*)g_buf : nullptr;
  a.ln_part = part ? (float*)g_buf : nullptr;
  a.part_stride = a.M;
  a.fin_eps = 1e-6f;
  return resid(a);
}
static GemmArgs with_patch(int P, int C, int64_t M, int g) {
  GemmArgs a = base(M, 256, C * P * P);
  a.patch_p = P;
  a.patch_g = g;
  a.patch_C = C;
  a.pos = (const float*)g_buf;
  return a;
}
static GemmArgs with_scales(GemmArgs a) {
  a.a_scale = a.w_scale = g_buf;
  return a;
}

int main() {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) return 77;  // a launch could succeed here: not on dummy buffers

  // ---- every variant against every epilogue ----
  for (int v = 21; v <= 32; ++v)
    for (int e = 0; e <= 9; ++e) run(NAME("sweep v%d epi%d", v, e), resid(base(300, 256, 128)), e, v);

  // ---- one feature at a time, on one variant of each family ----
  const int fam[] = {22, 25, 26, 29};
  for (int v : fam) {
    for (int e : {0, 1, 2, 4}) {
      GemmArgs a = resid(base(300, 256, 128));
      a.out_f32 = 1;
      run(NAME("out_f32 v%d epi%d", v, e), a, e, v);
    }
    for (int e : {0, 2}) {
      GemmArgs a = resid(base(300, 256, 128));
      a.resid32 = (const float*)g_buf;
      a.C32 = (float*)g_buf;
      run(NAME("resid32+C32 v%d epi%d", v, e), a, e, v);
    }
    {
      GemmArgs a = resid(base(300, 256, 128));
      a.resid32 = (const float*)g_buf;
      run(NAME("resid32 without C32 v%d", v), a, EPI_BIAS_RESID, v);
      a.resid32 = nullptr;
      a.C32 = (float*)g_buf;
      run(NAME("C32 without resid32 v%d", v), a, EPI_BIAS_RESID, v);
      a.resid32 = (const float*)g_buf;
      a.win_ws = 4;
      a.win_g = 10;
      run(NAME("resid32+C32+win_ws v%d", v), a, EPI_BIAS_RESID, v);
    }
    {
      GemmArgs a = resid(base(288, 256, 128));
      a.win_ws = 4;
      a.win_g = 10;
      run(NAME("win_ws v%d", v), a, EPI_BIAS_RESID, v);
    }
    {
      GemmArgs a = base(300, 256, 64);
      a.a_rpg = 2;
      a.a_gs = 384;
      a.a_is = 64;
      run(NAME("a_rpg v%d", v), a, EPI_BIAS, v);
      a.out_f32 = 1;
      run(NAME("a_rpg+out_f32 v%d", v), a, EPI_BIAS, v);
    }
    for (int P : {8, 16, 32}) run(NAME("patch_p %d v%d", P, v), with_patch(P, 3, 256, 2), EPI_PATCH, v);
    run(NAME("patch_p 14 v%d", v), with_patch(14, 16, 256, 2), EPI_PATCH, v);
    run(NAME("patch_p 16 epi0 v%d", v), with_patch(16, 3, 256, 2), EPI_BIAS, v);
    {
      GemmArgs a = with_patch(16, 3, 256, 2);
      a.K += 64;
      a.lda = a.ldw = a.K;
      run(NAME("patch_p K != C*P*P v%d", v), a, EPI_PATCH, v);
      a = with_patch(16, 3, 256, 2);
      a.A = g_buf + 8;
      run(NAME("patch_p misaligned A v%d", v), a, EPI_PATCH, v);
      a = with_patch(16, 3, 258, 2);
      run(NAME("patch_p M %% g*g v%d", v), a, EPI_PATCH, v);
      a = with_patch(16, 3, 256, 0);
      run(NAME("patch_p g 0 v%d", v), a, EPI_PATCH, v);
      a = with_patch(16, 3, 256, 2);
      a.a_rpg = 2;
      run(NAME("patch_p+a_rpg v%d", v), a, EPI_PATCH, v);
    }
    {
      GemmArgs a = base(300, 72, 128);
      a.ln_part = (float*)g_buf;
      a.part_stride = 300;
      run(NAME("ln_part N %% 64 v%d", v), a, EPI_BIAS, v);
      a = base(300, 128, 128);
      a.ln_part = (float*)g_buf;
      a.part_stride = 300;
      run(NAME("ln_part v%d", v), a, EPI_BIAS, v);
    }
    for (int groups : {0, 1, 16, 17}) run(NAME("ln_cpart groups %d v%d", groups, v), with_cpart(base(300, 256, 128), groups), EPI_BIAS, v);
    {
      GemmArgs a = with_cpart(base(300, 256, 128), 2);
      a.ln_stats = (const float*)g_buf;
      run(NAME("ln_cpart+ln_stats v%d", v), a, EPI_BIAS, v);
      run(NAME("ln_cpart resid epilogue v%d", v), with_cpart(resid(base(300, 256, 128)), 2), EPI_BIAS_RESID, v);
      a = resid(base(300, 256, 128));
      a.ln_stats = (const float*)g_buf;
      a.colsum = (const float*)g_buf;
      run(NAME("ln_stats resid epilogue v%d", v), a, EPI_BIAS_RESID, v);
      run(NAME("ln_stats v%d", v), a, EPI_BIAS_GELU, v);
    }
  }
  for (int v : {22, 23, 24, 25, 26, 27, 28, 29, 31}) {
    run(NAME("fin_stats v%d", v), with_fin(base(300, 256, 128), true, true), EPI_BIAS_RESID, v);
    run(NAME("fin_stats without fin_cnt v%d", v), with_fin(base(300, 256, 128), false, true), EPI_BIAS_RESID, v);
  }
  run("fin_stats without ln_part v26", with_fin(base(300, 256, 128), true, false), EPI_BIAS_RESID, 26);
  run("fin_stats epi0 v26", with_fin(base(300, 256, 128), true, true), EPI_BIAS, 26);
  run("fin_stats N % 64 v26", with_fin(base(300, 264, 128), true, false), EPI_BIAS_RESID, 26);
  {
    GemmArgs a = with_fin(base(288, 256, 128), true, true);
    a.win_ws = 4;
    a.win_g = 10;
    run("fin_stats+win_ws v26", a, EPI_BIAS_RESID, 26);
    a = with_fin(base(300, 256, 128), true, true);
    a.resid32 = (const float*)g_buf;
    a.C32 = (float*)g_buf;
    run("fin_stats+resid32 v26", a, EPI_BIAS_RESID, 26);
  }

  // ---- the 32-bit limits ----
  for (int v : fam) {
    GemmArgs a = base(300, 256, 128);
    a.ldc = (int64_t)1 << 24;
    run(NAME("ldc 2^24 v%d", v), a, EPI_BIAS, v);
    a.ldc = ((int64_t)1 << 24) - 8;
    run(NAME("ldc 2^24-8 v%d", v), a, EPI_BIAS, v);
    a = resid(base((int64_t)1 << 31, 256, 128));
    run(NAME("M 2^31 resid v%d", v), a, EPI_BIAS_RESID, v);
    run(NAME("M 2^31 epi0 v%d", v), a, EPI_BIAS, v);
    a.M -= 1;
    run(NAME("M 2^31-1 resid v%d", v), a, EPI_BIAS_RESID, v);
    run(NAME("nwg overflow v%d", v), base((int64_t)1 << 40, 256, 128), EPI_BIAS, v);
  }

  // ---- launch_gemm's own shape rules ----
  run("K % 64", base(300, 256, 96), EPI_BIAS, 26);
  run("K 0", base(300, 256, 0), EPI_BIAS, 26);
  run("N % 8", base(300, 60, 128), EPI_BIAS, 26);
  run("N 8", base(300, 8, 128), EPI_BIAS, 26);
  run("swiglu N % 64", base(300, 72, 128), EPI_SWIGLU, 26);
  run("swiglu N 128", base(300, 128, 128), EPI_SWIGLU, 26);
  run("M 0", base(0, 256, 128), EPI_BIAS, 26);
  run("M -1", base(-1, 256, 128), EPI_BIAS, 26);
  run("variant 126 (ablation encoding: tuning builds only)", base(300, 256, 128), EPI_BIAS, 126);
  run("variant 5026 (gn encoding: tuning builds only)", base(300, 256, 128), EPI_BIAS, 5026);

  // ---- MX-fp8 ----
  for (int v = 0; v <= 3; ++v) {
    run(NAME("mx v%d", v), with_scales(base(300, 256, 128)), EPI_BIAS, v, true);
    run(NAME("mx without scales v%d", v), base(300, 256, 128), EPI_BIAS, v, true);
    GemmArgs a = base(300, 256, 128);
    a.a_scale = g_buf;
    run(NAME("mx a_scale only v%d", v), a, EPI_BIAS, v, true);
    a.a_scale = nullptr;
    a.w_scale = g_buf;
    run(NAME("mx w_scale only v%d", v), a, EPI_BIAS, v, true);
  }
  for (int e = 0; e <= 9; ++e) {
    GemmArgs a = with_scales(resid(base(300, 256, 128)));
    run(NAME("mx epi%d", e), a, e, 0, true);
    a.c_scale = g_buf;
    run(NAME("mx c_scale epi%d", e), a, e, 0, true);
  }
  {
    GemmArgs a = with_scales(base(300, 256, 128));
    a.a_rpg = 2;
    run("mx a_rpg", a, EPI_BIAS, 0, true);
    a = with_scales(base(300, 256, 128));
    a.out_f32 = 1;
    run("mx out_f32", a, EPI_BIAS, 0, true);
    a = with_scales(base(288, 256, 128));
    a.win_ws = 4;
    a.win_g = 10;
    run("mx win_ws", a, EPI_BIAS, 0, true);
    a = with_scales(base(300, 256, 128));
    a.ln_stats = (const float*)g_buf;
    run("mx ln_stats", a, EPI_BIAS, 0, true);
    a = with_scales(base(300, 256, 128));
    a.ln_part = (float*)g_buf;
    a.part_stride = 300;
    run("mx ln_part", a, EPI_BIAS_RESID, 0, true);
    run("mx K % 64", with_scales(base(300, 256, 96)), EPI_BIAS, 0, true);
    run("mx N % 64", with_scales(base(300, 72, 128)), EPI_BIAS, 0, true);
    run("mx M 0", with_scales(base(0, 256, 128)), EPI_BIAS, 0, true);
    run("mx M 2^31", with_scales(base((int64_t)1 << 31, 256, 128)), EPI_BIAS, 0, true);
    run("mx M 2^31-1", with_scales(base(((int64_t)1 << 31) - 1, 256, 128)), EPI_BIAS, 0, true);
    run("mx nwg overflow", with_scales(base(((int64_t)1 << 31) - 1, 1 << 20, 128)), EPI_BIAS, 2, true);
  }

  // ---- variant 31: one case per line of gemm_8p_eligible (256 CUs assumed without a device: 512 tiles fill two rounds) ----
  {
    const int64_t M = 16384;
    const int N = 2048, K = 256;
    auto b8 = [&] { return base(M, N, K); };
    GemmArgs a;
    for (int e = 0; e <= 9; ++e) run(NAME("8p epi%d", e), resid(b8()), e, 31);
    a = b8(); a.out_f32 = 1; run("8p out_f32", a, EPI_BIAS, 31);
    a = b8(); a.win_ws = 4; a.win_g = 10; run("8p win_ws", a, EPI_BIAS, 31);
    a = b8(); a.a_rpg = 2; run("8p a_rpg", a, EPI_BIAS, 31);
    a = b8(); a.patch_p = 16; a.patch_g = 2; a.patch_C = 1; run("8p patch_p", a, EPI_BIAS, 31);
    a = b8(); a.ln_part = (float*)g_buf; run("8p ln_part", a, EPI_BIAS, 31);
    a = with_cpart(b8(), 4); run("8p ln_cpart", a, EPI_BIAS, 31);
    a = b8(); a.w_interleaved = 1; run("8p w_interleaved", a, EPI_BIAS, 31);
    a = b8(); a.resid32 = (const float*)g_buf; run("8p resid32", a, EPI_BIAS, 31);
    a = b8(); a.C32 = (float*)g_buf; run("8p C32", a, EPI_BIAS, 31);
    a = b8(); a.omap.rpg = 197; run("8p omap", a, EPI_BIAS, 31);
    a = b8(); a.a_scale = g_buf; run("8p a_scale", a, EPI_BIAS, 31);
    a = b8(); a.w_scale = g_buf; run("8p w_scale", a, EPI_BIAS, 31);
    a = b8(); a.c_scale = g_buf; run("8p c_scale", a, EPI_BIAS, 31);
    run("8p N % 256", base(M, N + 128, K), EPI_BIAS, 31);
    run("8p K % 128", base(M, N, 320), EPI_BIAS, 31);
    run("8p K 128", base(M, N, 128), EPI_BIAS, 31);
    run("8p ragged M without a_rows", base(M - 100, N, K), EPI_BIAS, 31);
    a = base(M - 100, N, K); a.a_rows = M - 1; run("8p ragged M, a_rows short", a, EPI_BIAS, 31);
    a = base(M - 100, N, K); a.a_rows = M; run("8p ragged M, a_rows cover the tile", a, EPI_BIAS, 31);
    a = b8(); a.lda = K - 8; run("8p lda < K", a, EPI_BIAS, 31);
    a = b8(); a.ldw = K - 8; run("8p ldw < K", a, EPI_BIAS, 31);
    a = b8(); a.ldc = N - 8; run("8p ldc < N", a, EPI_BIAS, 31);
    a = b8(); a.ln_stats = (const float*)g_buf; run("8p ln_stats without colsum", a, EPI_BIAS, 31);
    a = b8(); a.colsum = (const float*)g_buf; run("8p colsum without ln_stats", a, EPI_BIAS, 31);
    a = b8(); a.ln_stats = a.colsum = (const float*)g_buf; run("8p ln_stats+colsum", a, EPI_BIAS_GELU, 31);
    a = b8(); a.ldc = 65536; run("8p C offsets 2^31", a, EPI_BIAS, 31);
    a = b8(); a.lda = 131072; run("8p A offsets 2^32", a, EPI_BIAS, 31);
    a = b8(); a.ldw = 1 << 20; run("8p W offsets 2^32", a, EPI_BIAS, 31);
    a = b8(); a.A = g_buf + 8; run("8p misaligned A", a, EPI_BIAS, 31);
    a = b8(); a.W = g_buf + 8; run("8p misaligned W", a, EPI_BIAS, 31);
    a = b8(); a.C = g_buf + 8; run("8p misaligned C", a, EPI_BIAS, 31);
    a = b8(); a.lda = K + 4; run("8p lda % 8", a, EPI_BIAS, 31);
    a = b8(); a.bias = nullptr; run("8p null bias", a, EPI_BIAS, 31);
    run("8p under two rounds", base(M / 2, N, K), EPI_BIAS, 31);
    run("8p last round 83 % full", base(256 * 80, N, K), EPI_BIAS, 31);
    run("8p last round 87.5 % full", base(256 * 84, N, K), EPI_BIAS, 31);
  }

  // ---- launch shapes ----
  for (int v : {26, 28, 22})
    for (int K : {768, 1024, 1536, 3072}) run(NAME("gn K %d v%d", K, v), base(4096, 3072, K), EPI_BIAS, v);
  for (int N : {768, 1024, 1280}) run(NAME("gn tiles_n %d", N / 256), base(4096, N, 768), EPI_BIAS, 26);
  for (int v : {0, 2})
    for (int K : {768, 1024, 1536, 3072, 6144}) run(NAME("mx gn K %d v%d", K, v), with_scales(base(4096, 3072, K)), EPI_BIAS, v, true);
  run("mx gn tiles_n 4", with_scales(base(4096, 1024, 768)), EPI_BIAS, 0, true);
  for (int64_t M : {62499, 62500}) {  // M * ldc * 2 bytes on both sides of 128e6
    GemmArgs a = base(M, 1024, 128);
    run(NAME("nt_store M %lld", (long long)M), a, EPI_BIAS, 26);
    run(NAME("nt_store M %lld with resid", (long long)M), resid(a), EPI_BIAS_RESID, 26);
    run(NAME("nt_store M %lld with resid, epi0", (long long)M), resid(a), EPI_BIAS, 26);
    run(NAME("nt_store M %lld v22", (long long)M), a, EPI_BIAS_GELU, 22);
    run(NAME("nt_store M %lld v31", (long long)M), a, EPI_BIAS, 31);
  }
  for (int v = 22; v <= 29; ++v) {
    run(NAME("lds v%d", v), base(1024, 1024, 256), EPI_BIAS, v);
    run(NAME("lds v%d ln_cpart", v), with_cpart(base(1024, 1024, 256), 4), EPI_BIAS, v);
    run(NAME("lds v%d resid, K > N (fc2)", v), resid(base(1024, 256, 1024)), EPI_BIAS_RESID, v);
  }
  for (int v = 0; v <= 2; ++v) run(NAME("mx lds v%d", v), with_scales(base(1024, 1024, 256)), EPI_BIAS, v, true);
  return 0;
}
