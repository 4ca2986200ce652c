#!/bin/bash
# Patch for tools/build_variant.sh (run inside the copy of csrc/): wall-clock stamps in k_espcn_pair's tile loop.
#   tools/build_variant.sh /tmp/libsrk_l1stamps.so tools/pair_l1_stamps.sh
#   SRK_LIB_PATH=/tmp/libsrk_l1stamps.so python tools/pair_l1_prof.py
# Lane 0 of every wave stores s_memrealtime (100 MHz) at seven points of each of its own tiles: 0 behind the staging
# signal, 1 in front of the first layer (staged tile awaited, bias read), 2 behind the first layer's MFMAs of rows 2 .. 9,
# 3 behind l1_store, its counter waits and the computed rows 0 .. 1 of a fresh tile, 4 behind the wait in front of the
# second layer, 5 behind the second layer, 6 behind the epilogue's stores.  A wave that skips a phase (dead rows) leaves
# its stamps zero.  Reading the counter waits for lgkmcnt(0), so a stamped kernel is a little slower than the product;
# none of this is in the product library.  DESIGN 15.7.
python3 - <<'PY'
s = open("conv_pair.hip").read()
STAMP = ('if (lane == 0 && blockIdx.x < 256 && own < 64) g_pair_l1_stamps[((blockIdx.x * 8 + wave) * 64 + own) * 8 + %d] = '
         '__builtin_amdgcn_s_memrealtime();\n')


def put(marker, k, before):
    global s
    assert s.count(marker) == 1, marker
    s = s.replace(marker, STAMP % k + marker if before else marker + STAMP % k)


s = s.replace("__device__ unsigned g_pair_timeouts = 0;\n",
              "__device__ unsigned g_pair_timeouts = 0;\n__device__ unsigned long long g_pair_l1_stamps[256 * 8 * 64 * 8];\n")
put("    lds_cnt_signal(cnt + 6 + grp);\n", 0, False)
put("    const int vr = B.OH - ty * PR_TH;\n", 1, True)
put("      l1_frags(nm, moff, a1);\n", 2, False)
put("    // -- second layer out of the ring and the kept rows", 3, True)
put("      lds_cnt_wait(cnt + sslot[0], 2u * (suse[0] + 1), dead);\n", 4, False)
put("      // -- epilogue: bias, ReLU, NHWC stores", 5, True)
put("        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, v), yr, (int)o, 0, 0);\n      }\n", 6, False)
s += '''
// copies the stamps out and clears them
extern "C" int srk_pair_l1_stamps(unsigned long long* out) {
  const size_t bytes = sizeof(unsigned long long) * 256 * 8 * 64 * 8;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(srk::g_pair_l1_stamps), bytes) != hipSuccess) return -1;
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(srk::g_pair_l1_stamps)) != hipSuccess) return -1;
  return hipMemset(p, 0, bytes) == hipSuccess ? 0 : -1;
}
'''
s = s.replace("namespace {\n\nconstexpr int PR_TH", "constexpr int PR_TH", 1)
s = s.replace("}  // namespace\n\n// -1: not this kernel's problem.", "// -1: not this kernel's problem.", 1)
open("conv_pair.hip", "w").write(s)
PY
