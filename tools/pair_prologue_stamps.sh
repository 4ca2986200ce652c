#!/bin/bash
# Patch for tools/build_variant.sh (run inside the copy of csrc/): wall-clock stamps in k_espcn_pair's prologue.
#   tools/build_variant.sh /tmp/libsrk_stamps.so tools/pair_prologue_stamps.sh
#   SRK_LIB_PATH=/tmp/libsrk_stamps.so python tools/pair_prologue_prof.py
# Thread 0 of every block (its first wave is the one that polls the max|x| rendezvous) stores s_memrealtime (100 MHz) at
# six points; vmcnt(0) in front of stamps 1 - 3, so that a phase is charged with the loads it issued.  DESIGN 15.4.
python3 - <<'PY'
s = open("conv_pair.hip").read()
STAMP = '  if (tid == 0 && blockIdx.x < 256) g_pair_stamps[blockIdx.x * 8 + %d] = __builtin_amdgcn_s_memrealtime();\n'
WAIT = '  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n'


def put(marker, k, before, wait):
    global s
    assert s.count(marker) == 1, marker
    text = (WAIT if wait else "") + STAMP % k
    s = s.replace(marker, text + marker if before else marker + "\n" + text.rstrip("\n"))


s = s.replace("__device__ unsigned g_pair_timeouts = 0;\n",
              "__device__ unsigned g_pair_timeouts = 0;\n__device__ unsigned long long g_pair_stamps[256 * 8];\n")
put("  uint2* xin = xin_all + grp * PR_XBUF;", 0, False, False)
put("  // ---- second layer's filter into LDS: a thread's nine loads", 1, True, True)
put("  // ---- first layer: chunk c1 = channels 32 c1", 2, True, True)
put("  // ---- max|x| of all blocks:", 3, True, True)
put("  __syncthreads();  // filter, counters and max|x| visible", 4, False, False)
put("  unsigned own = 0;  // own tiles done", 5, True, False)
s += '''
extern "C" int srk_pair_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(srk::g_pair_stamps), 256 * 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
'''
s = s.replace("namespace {\n\nconstexpr int PR_TH", "constexpr int PR_TH", 1)
s = s.replace("}  // namespace\n\n// -1: not this kernel's problem.", "// -1: not this kernel's problem.", 1)
open("conv_pair.hip", "w").write(s)
PY
