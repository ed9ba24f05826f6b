// api_numeric.cpp -- C-ABI entry point of NumericToString; stateless.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/numeric_to_string.cpp:18-92.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "numeric_kernels.hpp"
#include "runtime.hpp"

using namespace ovtk;

namespace {

constexpr uint32_t kStopFlags = kFlagOutCapacity | kFlagTooLong;

struct NumType {
    int size;      // bytes of an element
    int longest;   // bytes of the type's longest text
};
// i8 "-128", i16 "-32768", i32 "-2147483648", i64 "-9223372036854775808", u8 "255", u16 "65535", u32 "4294967295",
// u64 "18446744073709551615", f32 "-3.40282e+38" / "-0.000123456", f64 "-1.79769e+308", boolean "false"
constexpr NumType kTypes[kNumTypes] = {{1, 4}, {2, 6}, {4, 11}, {8, 20}, {1, 3}, {2, 5}, {4, 10}, {8, 20}, {4, 12}, {8, 13}, {1, 5}};
static_assert(OVTK_NUM_I8 == kNumI8 && OVTK_NUM_I64 == kNumI64 && OVTK_NUM_U8 == kNumU8 && OVTK_NUM_U64 == kNumU64 && OVTK_NUM_F32 == kNumF32 &&
                  OVTK_NUM_F64 == kNumF64 && OVTK_NUM_BOOL == kNumBool,
              "the kernels' type numbers are the header's");

// The powers of ten of the float path: built once per process (exact big-integer arithmetic, numeric_table.hpp), one device copy per
// device, kept until the process ends.
int pow10_table(int device, const NumPow10** dev) {
    static std::mutex mu;
    static std::vector<NumPow10> host;
    static std::map<int, std::unique_ptr<DevBuf>> tables;
    std::lock_guard<std::mutex> lk(mu);
    auto& t = tables[device];
    if (!t) {
        if (host.empty() && !build_num_pow10_table(host)) {
            host.clear();
            return set_error(OVTK_E_UNSUPPORTED, "NumericToString: the power-of-ten table failed its own check");
        }
        auto buf = std::make_unique<DevBuf>();
        if (int rc = buf->upload(host.data(), host.size() * sizeof(NumPow10))) return rc;
        OVTK_HIP(hipStreamSynchronize(nullptr));
        t = std::move(buf);
    }
    *dev = t->as<NumPow10>();
    return OVTK_OK;
}

template <int DT>
void launch_count(LaunchLog& marks, hipStream_t s, int grid, const NumIn& in, uint8_t* lens) {
    OVTK_LAUNCH(marks, "numeric_count", num_count_kernel<DT>, grid, kBlockThreads, s, in, lens);
}
template <int DT>
void launch_write(LaunchLog& marks, hipStream_t s, int grid, const NumIn& in, const int32_t* begins, uint8_t* chars, const RunStatus* st) {
    OVTK_LAUNCH(marks, "numeric_to_string", num_write_kernel<DT>, grid, kBlockThreads, s, in, begins, chars, st, kStopFlags);
}
#define OVTK_NUM_DISPATCH(dtype, call)                   \
    switch (dtype) {                                     \
        case kNumI8: call(kNumI8); break;                \
        case kNumI16: call(kNumI16); break;              \
        case kNumI32: call(kNumI32); break;              \
        case kNumI64: call(kNumI64); break;              \
        case kNumU8: call(kNumU8); break;                \
        case kNumU16: call(kNumU16); break;              \
        case kNumU32: call(kNumU32); break;              \
        case kNumU64: call(kNumU64); break;              \
        case kNumF32: call(kNumF32); break;              \
        case kNumF64: call(kNumF64); break;              \
        default: call(kNumBool); break;                  \
    }

}  // namespace

extern "C" {

int64_t ovtk_numeric_to_string_bound(int dtype, int64_t n) {
    if (dtype < 0 || dtype >= kNumTypes || n < 0) return -1;
    return n * kTypes[dtype].longest;
}

int ovtk_numeric_to_string(const void* in, int dtype, int64_t n, ovtk_strings_out* out, int mem, int device, void* stream) {
    if (dtype < 0 || dtype >= kNumTypes) return set_error(OVTK_E_ARG, "NumericToString: unsupported input type " + std::to_string(dtype));   // :88
    if (n < 0) return set_error(OVTK_E_ARG, "numeric_to_string: negative size");
    if (n > 0 && !in) return set_error(OVTK_E_ARG, "numeric_to_string: null input");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (!out || out->chars_capacity < 0) return set_error(OVTK_E_ARG, "numeric_to_string: bad output");
    if (n > 0 && (!out->begins || !out->ends)) return set_error(OVTK_E_ARG, "numeric_to_string: null output offsets");
    const NumType ty = kTypes[dtype];
    if (reinterpret_cast<uintptr_t>(in) % size_t(ty.size)) return set_error(OVTK_E_ARG, "numeric_to_string: the input is not aligned to its element size");
    if (n >= (int64_t(1) << 31) / ty.longest + 1 || n * ty.longest >= (int64_t(1) << 31))
        return set_error(OVTK_E_UNSUPPORTED, "NumericToString: the text could reach 2^31 bytes; split the call");
    if (int rc = use_device(device)) return rc;
    out->n_chars = 0;
    if (n == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    NumIn p{};
    p.n = n;
    if (dtype == kNumF32 || dtype == kNumF64) {
        if (int rc = pow10_table(device, &p.tab)) return rc;
        // (measurements and tests: every finite element through the exact big-integer comparison)
        const char* force = std::getenv("OVTK_NUM2STR_EXACT");
        p.force_exact = force && force[0] == '1' ? 1 : 0;
    }
    WorkspaceLease ws(device);
    if (!ws->host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws->status.ensure(sizeof(RunStatus))) return rc;
    RunStatus* st = ws->status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(st, 0, sizeof(RunStatus), s));
    const uint8_t* d_in = nullptr;
    if (int rc = in_source(ws->in_chars, static_cast<const uint8_t*>(in), size_t(n) * size_t(ty.size), mem, s, &d_in)) return rc;
    p.data = d_in;
    if (int rc = ws->gen[0].ensure(size_t(n))) return rc;
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(n))) return rc;
    uint8_t* lens = ws->gen[0].as<uint8_t>();
    int32_t *d_b = nullptr, *d_e = nullptr;
    uint8_t* d_c = nullptr;
    if (int rc = out_target(ws->out_a, out->begins, size_t(n) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_b, out->ends, size_t(n) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_c, out->chars, size_t(out->chars_capacity), mem, &d_c)) return rc;
    const long long cap = std::min<long long>(out->chars_capacity, INT32_MAX - 1);
    const int grid = int((n + kBlockThreads - 1) / kBlockThreads);   // a lane per element, a wave per 64 consecutive ones

#define OVTK_NUM_COUNT(DT) launch_count<DT>(ws->marks, s, grid, p, lens)
    OVTK_NUM_DISPATCH(dtype, OVTK_NUM_COUNT)
#undef OVTK_NUM_COUNT
    launch_scan(ws->marks, "numeric_offsets", s, n, NumLen{lens}, NumOffsets{d_b, d_e}, NumFin{st, cap}, ws->tiles.as<long long>(), st, kStopFlags);
#define OVTK_NUM_WRITE(DT) launch_write<DT>(ws->marks, s, grid, p, d_b, d_c, st)
    OVTK_NUM_DISPATCH(dtype, OVTK_NUM_WRITE)
#undef OVTK_NUM_WRITE
    if (int rc = finish_status(*ws.ws, s)) return rc;
    const RunStatus& h = *ws->host_status;
    if (h.flags & kFlagTooLong) return set_error(OVTK_E_UNSUPPORTED, "NumericToString: the text would reach 2^31 bytes; split the call");
    out->n_chars = h.n_out;
    if (h.flags & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, "NumericToString: output chars buffer too small (" + std::to_string(h.n_out) + " bytes, capacity " +
                                              std::to_string(out->chars_capacity) + ")");
    int e = 0;
    e = e ? e : copy_back(out->begins, d_b, size_t(n) * 4, mem, s);
    e = e ? e : copy_back(out->ends, d_e, size_t(n) * 4, mem, s);
    e = e ? e : copy_back(out->chars, d_c, size_t(out->n_chars), mem, s);
    if (e) return e;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

}  // extern "C"
