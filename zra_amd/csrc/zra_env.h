// zra_amd — the environment variables the library reacts to, and the only place that reads them.
// Every name is read through the three functions below; tests/test_env_knobs.py holds this list and the call sites to each other.
//
// Operational (documented in INTEGRATION.md):
//   ZRA_DEVICE              HIP device of the engine pool
//   ZRA_ENGINES             engines of the pool (1-64)
//   ZRA_SCRATCH_CAP_GIB     device scratch the pool's idle engines may keep
//   ZRA_STREAM_AHEAD_MIB    decode-ahead window of the streaming random-access reader (read per call)
//   ZRA_HOST_CHUNK_MIB      chunk of the host-pointer calls (read per call)
//   ZRA_COMM_CHUNK_MIB      largest piece of one RCCL message
//   ZRA_DEC_SMALL_MAX       largest decode pass the one-launch kernel takes
// Test hooks (a test in tests/ sets each, to put a path that default calls of other sizes take onto small inputs):
//   ZRA_ALLOC_LIMIT_MIB     any single scratch reservation above it fails
//   ZRA_ENC_BUDGET_GIB      scratch budget per context of the encoder's batch path (read per call)
//   ZRA_ENC_FAIL_BATCH      the batch path gives up behind this batch (read per call)
//   ZRA_ENC_POISON          table scratch filled with 0xA5 before every batch
//   ZRA_MF_LS               0: no LDS-source dfast kernel
//   ZRA_MF_LS_MAX           largest call of the LDS-source dfast kernel, in frames
//   ZRA_MF_WAVES            match-finder waves per CU of the persistent pipeline
//   ZRA_MF_FLAGS            0: no bucket flags in the dfast table kernel
//   ZRA_MF_EPOCH            epoch bits of the dfast table cells (0: tables cleared per frame)
//   ZRA_ENT_WGS             entropy workgroups per CU of the persistent pipeline
//   ZRA_ENT_SPLIT           split entropy stage: 0 never, 1 calls of >= 256 frames, 2 always
//   ZRA_DEC_FMB             0: no block-parallel decode pass
//   ZRA_DEC_FMB_MIN         smallest pass that takes the block-parallel decode pass, in jobs
//   ZRA_DEC_FRONT           0: the parse wave leaves every Huffman-coded literal section to the Huffman kernel
//   ZRA_DEC_CHAIN_LDS       decoder's LDS-table chain kernel: 0 never, 1 beside the other one, 2 alone
//   ZRA_DEC_CHAIN_LDS_MIN   smallest round that runs the LDS-table chain kernel, in jobs
//   ZRA_COMM_CHUNK_BYTES    largest piece of one RCCL message, in bytes
// Diagnostics (stderr only):
//   ZRA_COMM_TRACE          a rank's local status when a collective call fails (read per call)
//   ZRA_ENC_TRACE           launch timeline of the persistent encoder pipeline
//   ZRA_RA_TRACE            host-side timeline of random-access calls
#pragma once
#include <cstdlib>

namespace zra_env {

inline bool env_set(const char* name) { return std::getenv(name) != nullptr; }
inline int env_int(const char* name, int dflt) { const char* s = std::getenv(name); return s ? std::atoi(s) : dflt; }
inline long long env_i64(const char* name, long long dflt) { const char* s = std::getenv(name); return s ? std::atoll(s) : dflt; }

}  // namespace zra_env
