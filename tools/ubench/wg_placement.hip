// Where do the waves of co-resident workgroups land?  (The shared table inversion of k_scalarmul_coz_unsat puts one
// wave per workgroup on duty per grid-stride iteration, wave iter & 3; if wave j of every workgroup of a CU sits on
// SIMD j, the four duty waves of a CU queue on one SIMD while three stand idle.  DESIGN.md 3.9.)
// The kernel has the ladder's launch shape -- 256 threads, __launch_bounds__(256, 4), 1 024 blocks -- and 36 KB of LDS,
// so that four workgroups fit a CU (160 KB) and a fifth does not, as the ladder's 128 VGPRs have it.  Every wave
// reads HW_REG_HW_ID and HW_REG_XCC_ID once and writes them with its block and wave index and the 100 MHz clock at
// its start and end; a fixed count of dependent multiply-adds in between (no waiting on anything) keeps every block
// of the grid resident at the same time, which the host checks from the clocks.
//   build: make -C tools/ubench wg_placement      run on the GPU box: tools/ubench/wg_placement <out.json>
// One process is one run; profiles/wg_placement.json holds a few.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <tuple>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); return 1; } } while (0)

constexpr int WG = 256, WAVES = WG / 64, BLOCKS = 1024, REC = 8;
constexpr int LDS_WORDS = 36 * 1024 / 4;

// s_getreg operand: id | offset << 6 | (size - 1) << 11
constexpr int GETREG_HW_ID = 4 | (31 << 11), GETREG_XCC_ID = 20 | (31 << 11);

__global__ void __launch_bounds__(WG, 4) k_where(uint32_t* __restrict__ out, uint32_t nrec, int spin, uint32_t seed) {
  __shared__ uint32_t pad[LDS_WORDS];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  const uint32_t hw = __builtin_amdgcn_s_getreg(GETREG_HW_ID), xcc = __builtin_amdgcn_s_getreg(GETREG_XCC_ID);
  for (uint32_t i = threadIdx.x; i < (uint32_t)LDS_WORDS; i += WG) pad[i] = i ^ seed;
  __syncthreads();
  uint32_t a = threadIdx.x * 2654435761u + seed;
  for (int it = 0; it < spin; ++it) a = a * 1664525u + pad[(a >> 8) % (uint32_t)LDS_WORDS];
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  const uint32_t rec = blockIdx.x * WAVES + wave;
  if ((threadIdx.x & 63u) == 0u && rec < nrec) {
    uint32_t* o = out + (size_t)rec * REC;
    o[0] = blockIdx.x;
    o[1] = wave;
    o[2] = hw;
    o[3] = xcc;
    o[4] = (uint32_t)t0;
    o[5] = (uint32_t)(t0 >> 32);
    o[6] = (uint32_t)(t1 - t0);
    o[7] = a;  // keeps the loop
  }
}

struct Wave { uint32_t block, wave, slot, simd, cu, sh, se, tg, xcc; uint64_t t0, t1; };

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "wg_placement.json";
  const int spin = argc > 2 ? atoi(argv[2]) : 20000;
  const uint32_t nrec = BLOCKS * WAVES;
  uint32_t* d;
  CK(hipMalloc(&d, (size_t)nrec * REC * sizeof(uint32_t)));
  CK(hipMemset(d, 0xff, (size_t)nrec * REC * sizeof(uint32_t)));
  k_where<<<BLOCKS, WG>>>(d, nrec, 16, 1u);  // warm-up: code object load
  CK(hipDeviceSynchronize());
  CK(hipMemset(d, 0xff, (size_t)nrec * REC * sizeof(uint32_t)));
  k_where<<<BLOCKS, WG>>>(d, nrec, spin, 2u);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<uint32_t> h((size_t)nrec * REC);
  CK(hipMemcpy(h.data(), d, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CK(hipFree(d));

  std::vector<Wave> w(nrec);
  uint64_t first_end = ~0ull, last_start = 0;
  for (uint32_t r = 0; r < nrec; ++r) {
    const uint32_t* o = &h[(size_t)r * REC];
    if (o[0] != r / WAVES || o[1] != r % WAVES) { printf("record %u was not written\n", r); return 1; }
    const uint32_t hw = o[2];
    Wave& v = w[r];
    v.block = o[0]; v.wave = o[1];
    v.slot = hw & 15u; v.simd = (hw >> 4) & 3u; v.cu = (hw >> 8) & 15u; v.sh = (hw >> 12) & 1u; v.se = (hw >> 13) & 7u;
    v.tg = (hw >> 16) & 15u; v.xcc = o[3] & 15u;
    v.t0 = ((uint64_t)o[5] << 32) | o[4]; v.t1 = v.t0 + o[6];
    first_end = std::min(first_end, v.t1); last_start = std::max(last_start, v.t0);
  }
  const bool all_resident = last_start < first_end;  // every wave had started before the first one ended

  // wave j of a workgroup -> SIMD
  unsigned simd_of_wave[WAVES][4] = {};
  unsigned distinct4 = 0, identity = 0;
  for (uint32_t b = 0; b < BLOCKS; ++b) {
    unsigned mask = 0; bool id = true;
    for (int j = 0; j < WAVES; ++j) {
      const Wave& v = w[b * WAVES + j];
      ++simd_of_wave[j][v.simd]; mask |= 1u << v.simd; id = id && v.simd == (uint32_t)j;
    }
    distinct4 += mask == 15u; identity += id;
  }
  // blocks per CU (all resident together when all_resident)
  using Key = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>;
  std::map<Key, std::vector<uint32_t>> cus;
  for (uint32_t b = 0; b < BLOCKS; ++b) {
    const Wave& v = w[b * WAVES];
    cus[Key(v.xcc, v.se, v.sh, v.cu)].push_back(b);
  }
  unsigned per_cu_hist[9] = {}, low2_distinct_hist[5] = {}, tg_low2_distinct_hist[5] = {}, tg_distinct = 0;
  // duty waves of a CU's workgroups on one SIMD: rule iter & 3 (wave j of each), rule (iter + block) & 3, and the
  // rule by placement, target SIMD (tg + iter) & 3
  unsigned clash_iter = 0, clash_block = 0, clash_tg = 0, pairs = 0;
  for (auto& kv : cus) {
    const auto& bl = kv.second;
    ++per_cu_hist[std::min<size_t>(bl.size(), 8)];
    unsigned m_low = 0, m_tg = 0, m_tgfull = 0;
    for (uint32_t b : bl) { m_low |= 1u << (b & 3u); m_tg |= 1u << (w[b * WAVES].tg & 3u); m_tgfull |= 1u << w[b * WAVES].tg; }
    ++low2_distinct_hist[__builtin_popcount(m_low)];
    ++tg_low2_distinct_hist[__builtin_popcount(m_tg)];
    tg_distinct += (size_t)__builtin_popcount(m_tgfull) == bl.size();
    for (uint32_t iter = 0; iter < 4; ++iter) {
      unsigned c_i[4] = {}, c_b[4] = {}, c_t[4] = {};
      for (uint32_t b : bl) {
        const Wave* wv = &w[b * WAVES];
        ++c_i[wv[iter & 3u].simd];
        ++c_b[wv[(iter + b) & 3u].simd];
        const uint32_t target = (wv[0].tg + iter) & 3u;
        uint32_t duty = iter & 3u;
        for (int j = WAVES - 1; j >= 0; --j) if (wv[j].simd == target) duty = (uint32_t)j;
        ++c_t[wv[duty].simd];
      }
      for (int s = 0; s < 4; ++s) {
        clash_iter += c_i[s] * (c_i[s] - 1) / 2; clash_block += c_b[s] * (c_b[s] - 1) / 2; clash_tg += c_t[s] * (c_t[s] - 1) / 2;
      }
      pairs += (unsigned)(bl.size() * (bl.size() - 1) / 2);
    }
  }

  FILE* f = fopen(path, "w");
  if (!f) { printf("cannot write %s\n", path); return 1; }
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  fprintf(f, "{\"device\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"blocks\": %d, \"threads\": %d, \"lds_bytes\": %d, \"spin\": %d,\n",
          prop.name, prop.gcnArchName, prop.multiProcessorCount, BLOCKS, WG, LDS_WORDS * 4, spin);
  fprintf(f, " \"all_blocks_resident_together\": %s, \"overlap_us\": %.1f,\n", all_resident ? "true" : "false", ((double)first_end - (double)last_start) * 0.01);
  fprintf(f, " \"simd_of_wave\": {");
  for (int j = 0; j < WAVES; ++j)
    fprintf(f, "\"wave%d\": [%u, %u, %u, %u]%s", j, simd_of_wave[j][0], simd_of_wave[j][1], simd_of_wave[j][2], simd_of_wave[j][3], j < WAVES - 1 ? ", " : "},\n");
  fprintf(f, " \"workgroups_on_four_distinct_simds\": %u, \"workgroups_with_wave_j_on_simd_j\": %u,\n", distinct4, identity);
  fprintf(f, " \"cus_seen\": %zu, \"workgroups_per_cu_hist\": [", cus.size());
  for (int i = 0; i < 9; ++i) fprintf(f, "%u%s", per_cu_hist[i], i < 8 ? ", " : "],\n");
  fprintf(f, " \"cus_by_distinct_block_low2\": [%u, %u, %u, %u, %u],\n", low2_distinct_hist[0], low2_distinct_hist[1], low2_distinct_hist[2], low2_distinct_hist[3], low2_distinct_hist[4]);
  fprintf(f, " \"cus_by_distinct_tg_id_low2\": [%u, %u, %u, %u, %u], \"cus_with_distinct_tg_ids\": %u,\n", tg_low2_distinct_hist[0], tg_low2_distinct_hist[1], tg_low2_distinct_hist[2], tg_low2_distinct_hist[3], tg_low2_distinct_hist[4], tg_distinct);
  fprintf(f, " \"duty_pairs_on_one_simd\": {\"of_pairs\": %u, \"iter\": %u, \"iter_plus_block\": %u, \"tg_plus_iter_by_simd\": %u},\n", pairs, clash_iter, clash_block, clash_tg);
  fprintf(f, " \"sample_cus\": [");
  int shown = 0;
  for (auto& kv : cus) {
    if (shown == 12) break;
    fprintf(f, "%s\n  {\"xcc\": %u, \"se\": %u, \"sh\": %u, \"cu\": %u, \"workgroups\": [", shown ? "," : "", std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), std::get<3>(kv.first));
    for (size_t i = 0; i < kv.second.size(); ++i) {
      const Wave* wv = &w[kv.second[i] * WAVES];
      fprintf(f, "%s{\"block\": %u, \"tg\": %u, \"simd\": [%u, %u, %u, %u], \"slot\": [%u, %u, %u, %u]}", i ? ", " : "", wv[0].block, wv[0].tg,
              wv[0].simd, wv[1].simd, wv[2].simd, wv[3].simd, wv[0].slot, wv[1].slot, wv[2].slot, wv[3].slot);
    }
    fprintf(f, "]}");
    ++shown;
  }
  fprintf(f, "]}\n");
  fclose(f);
  printf("wg_placement: resident together %d, wave j on SIMD j in %u of %d workgroups, duty pairs on one SIMD: iter %u, iter+block %u, placement %u of %u\n",
         (int)all_resident, identity, BLOCKS, clash_iter, clash_block, clash_tg, pairs);
  return 0;
}
