// cgx_variant.h — the SpMV variant: its bits, the forms that have a kernel,
// and the lists every instantiation, switch and request check derives from
// (DESIGN.md §4 has the same tables in prose).
//
// A variant is a public int (cgx_csr_set_variant, cgx_csr_variant,
// $CGX_SPMV_VARIANT, the autotune record, the bench JSON, the profile logs):
// the static_asserts at the end pin every name to its decimal, and read the
// other way they are the dictionary from a logged number to its form.
#pragma once

namespace cgx {

// ---- the bits ---------------------------------------------------------------
// CSR-stream (no SELL bit): a workgroup stages a row block in LDS
constexpr int kXcd = 1;     // XCD-contiguous split of the row blocks / slices
constexpr int kNt = 2;      // non-temporal val / col (SELL: value / code) loads
constexpr int kPair = 4;    // paired 16-B value / 8-B column loads
constexpr int kPipe = 8;    // software-pipelined loop (CSR-stream: paired loads only;
                            // dictionary SELL: 1 row per lane, slices <= 8 wide)
constexpr int kAblG = 16;   // timing ablation, cgx_tune_spmv only: no gathers
constexpr int kAblR = 32;   // timing ablation, cgx_tune_spmv only: no LDS / row phase
constexpr int kC16 = 128;   // 16-bit column deltas on the paired loop: 10 B per entry, not 12
constexpr int kQuad = 256;  // quad loads (4-entry alignment), pipelined
// the SELL copies (cgx_internal.h SellSlice): one wave per slice
constexpr int kSell = 2048;     // dictionary SELL-64
constexpr int kSell2 = 4096;    // ... with 2 rows per lane (slices of 128 rows)
constexpr int kSellP = 8192;    // SELL-P: a pattern per slice, a slot mask per row
constexpr int kMask32 = 16384;  // SELL-P with u32 row masks (u8 otherwise)
constexpr int kVc = 32768;      // SELL-P value codes: one code byte per slot
constexpr int kVc4 = 262144;    // 4-bit value codes (at most kVc4Max values)
constexpr int kVcPipe = 524288;  // software-pipelined value-code walk (slices <= 8 wide)
constexpr int kVcSt = 1048576;   // stencil slices: offsets -1 / +1 by lane shifts
constexpr int kMarch = 2097152;  // plane march: slices a plane apart in turn
constexpr int kVT = 8388608;     // value-code templates: frequent code chunks from LDS
constexpr int kVL = 33554432;    // lean stencil walk: a class byte per slice, no row data
// CSR-stream on the interleaved val / col copy (pipelined paired loop only)
constexpr int kIL = 67108864;
// Retired, no constant: 64 (half tile), 512 (wave tile), 65536 and 131072
// (value-code occupancy / half-chunk forms), 16777216 (y-march). No form
// carries them; a request with one of them is refused or, inside a SELL
// request's mask, dropped like any unknown bit.

// ---- the forms --------------------------------------------------------------
constexpr int kCsrPair = kPair | kXcd;          // 5
constexpr int kCsrPipe = kPipe | kPair | kXcd;  // 13: the production CSR-stream form
constexpr int kCsrQuad = kQuad | kPipe;         // 264
constexpr int kFSell2 = kSell | kSell2;         // 6144
constexpr int kFSellP32 = kSellP | kMask32;     // 24576
// value-code SELL-P and its loops
constexpr int kFVc = kSellP | kVc;              // 40960
constexpr int kFVc4 = kFVc | kVc4;              // 303104
constexpr int kFVcPipe = kFVc | kVcPipe;        // 565248
constexpr int kFVc4Pipe = kFVc4 | kVcPipe;      // 827392
constexpr int kFVcSt = kFVcPipe | kVcSt;        // 1613824
constexpr int kFVc4St = kFVc4Pipe | kVcSt;      // 1875968
constexpr int kFVcMarch = kFVcSt | kMarch;      // 3710976
constexpr int kFVc4March = kFVc4St | kMarch;    // 3973120
constexpr int kFVc4PipeT = kFVc4Pipe | kVT;     // 9216000
constexpr int kFVc4StT = kFVc4St | kVT;         // 10264576
constexpr int kFVc4MarchT = kFVc4March | kVT;   // 12361728
// the lean walk's request (kVL | kVlBase) and its generic slices' form
constexpr int kVlBase = kSell | kNt | kVc | kVc4 | kVcPipe | kVcSt | kVT;
// every bit a request on a SELL copy may carry (cgx_csr_set_variant)
constexpr int kSellBits = kNt | kAblG | kSell | kSell2 | kSellP | kMask32 | kVc | kVc4 |
                          kVcPipe | kVcSt | kMarch | kVT;
// the CSR-stream bits spmv_variant keeps (kC16 and kIL it re-adds itself)
constexpr int kCsrBits = kXcd | kNt | kPair | kPipe | kAblG | kAblR | kQuad;

// ---- predicates -------------------------------------------------------------
// the variant runs on a SELL copy (dictionary SELL or SELL-P)
constexpr bool sell_variant(int v) { return (v & (kSell | kSellP)) != 0; }
// CSR-stream form (mode 2's SpMV reads p through the cache: one barrier)
constexpr bool csr_stream_variant(int v) { return !sell_variant(v); }

// ---- the lists (X-macros) ---------------------------------------------------
// families: a form plain and non-temporal; and with / without the XCD split
#define CGX_F_NT(X, F) X(F) X(F | kNt)
#define CGX_F_XN(X, F) CGX_F_NT(X, F) CGX_F_NT(X, F | kXcd)

#define CGX_CSR_FORMS(X)                                                                 \
  CGX_F_XN(X, 0) CGX_F_XN(X, kPair) CGX_F_XN(X, kPipe | kPair) CGX_F_XN(X, kCsrQuad)     \
  CGX_F_NT(X, kCsrPair | kC16) CGX_F_NT(X, kCsrPipe | kIL)
// dictionary SELL: 1 and 2 rows per lane, and the pipelined 1-row form
#define CGX_SELL_FORMS(X) CGX_F_NT(X, kSell) CGX_F_NT(X, kFSell2)
#define CGX_SELL_PIPE_FORMS(X) CGX_F_NT(X, kSell | kPipe)
#define CGX_SELLP_FORMS(X) CGX_F_NT(X, kSellP)
#define CGX_SELLP32_FORMS(X) CGX_F_NT(X, kFSellP32)
// value codes: the walks in slice (or list) order, and the plane marches
#define CGX_VC_WALK_FORMS(X)                                                             \
  CGX_F_NT(X, kFVc) CGX_F_NT(X, kFVc4) CGX_F_NT(X, kFVcPipe) CGX_F_NT(X, kFVc4Pipe)      \
  CGX_F_NT(X, kFVcSt) CGX_F_NT(X, kFVc4St) CGX_F_NT(X, kFVc4PipeT) CGX_F_NT(X, kFVc4StT)
#define CGX_VC_MARCH_FORMS(X)                                                            \
  CGX_F_NT(X, kFVcMarch) CGX_F_NT(X, kFVc4March) CGX_F_NT(X, kFVc4MarchT)

// every form k_spmv_dot is instantiated for; cgx_csr_set_variant accepts these
#define CGX_SPMV_LIST(X)                                                                 \
  CGX_CSR_FORMS(X) CGX_SELL_FORMS(X) CGX_SELL_PIPE_FORMS(X) CGX_SELLP_FORMS(X)           \
  CGX_SELLP32_FORMS(X) CGX_VC_WALK_FORMS(X) CGX_VC_MARCH_FORMS(X)
// mode 4 (k_spmv_fd): the production forms only, f64 only
#define CGX_FD_LIST(X)                                                                   \
  CGX_F_NT(X, kCsrPipe) CGX_SELLP_FORMS(X) CGX_VC_WALK_FORMS(X) CGX_VC_MARCH_FORMS(X)
// mode 2 (k_spmv_fused): mode 4's forms, plain CSR-stream and the dictionary
// SELL forms small matrices take
#define CGX_FUSED_LIST(X)                                                                \
  CGX_FD_LIST(X) X(0) X(kCsrPair) X(kCsrPair | kC16) X(kCsrQuad | kXcd) CGX_SELL_FORMS(X) \
  CGX_SELL_PIPE_FORMS(X) CGX_SELLP32_FORMS(X)
// the interior SpMV with the halo push in front and the boundary launch
// (k_spmv_dot_push, k_spmv_dot_bnd): the SELL forms a partitioned matrix
// takes (slice lists: no plane march)
#define CGX_PUSH_LIST(X)                                                                 \
  CGX_SELL_FORMS(X) CGX_SELLP_FORMS(X) CGX_SELLP32_FORMS(X) CGX_VC_WALK_FORMS(X)
// CSR-stream timing ablations: cgx_tune_spmv only
#define CGX_ABLATION_LIST(X)                                                             \
  X(kCsrPipe | kNt | kAblG) X(kCsrPipe | kNt | kAblR) X(kCsrPipe | kNt | kAblG | kAblR)  \
  X(kCsrPipe | kNt | kAblG | kAblR | kIL) X(kCsrPipe | kNt | kAblR | kIL)

// ---- the public decimals ----------------------------------------------------
#define CGX_PIN(name, dec) static_assert((name) == dec, "public variant number moved")
CGX_PIN(kXcd, 1); CGX_PIN(kNt, 2); CGX_PIN(kPair, 4); CGX_PIN(kPipe, 8);
CGX_PIN(kAblG, 16); CGX_PIN(kAblR, 32); CGX_PIN(kC16, 128); CGX_PIN(kQuad, 256);
CGX_PIN(kSell, 2048); CGX_PIN(kSell2, 4096); CGX_PIN(kSellP, 8192); CGX_PIN(kMask32, 16384);
CGX_PIN(kVc, 32768); CGX_PIN(kVc4, 262144); CGX_PIN(kVcPipe, 524288);
CGX_PIN(kVcSt, 1048576); CGX_PIN(kMarch, 2097152); CGX_PIN(kVT, 8388608);
CGX_PIN(kVL, 33554432); CGX_PIN(kIL, 67108864);
// CSR-stream
CGX_PIN(kXcd | kNt, 3); CGX_PIN(kPair | kXcd, 5); CGX_PIN(kPair | kNt, 6);
CGX_PIN(kPair | kXcd | kNt, 7); CGX_PIN(kPipe | kPair, 12); CGX_PIN(kCsrPipe, 13);
CGX_PIN(kPipe | kPair | kNt, 14); CGX_PIN(kCsrPipe | kNt, 15);
CGX_PIN(kCsrQuad, 264); CGX_PIN(kCsrQuad | kXcd, 265); CGX_PIN(kCsrQuad | kNt, 266);
CGX_PIN(kCsrQuad | kXcd | kNt, 267);
CGX_PIN(kCsrPair | kC16, 133); CGX_PIN(kCsrPair | kC16 | kNt, 135);
CGX_PIN(kCsrPipe | kIL, 67108877); CGX_PIN(kCsrPipe | kIL | kNt, 67108879);
// dictionary SELL, SELL-P
CGX_PIN(kSell | kNt, 2050); CGX_PIN(kSell | kPipe, 2056); CGX_PIN(kSell | kPipe | kNt, 2058);
CGX_PIN(kFSell2, 6144); CGX_PIN(kFSell2 | kNt, 6146);
CGX_PIN(kSellP | kNt, 8194); CGX_PIN(kFSellP32, 24576); CGX_PIN(kFSellP32 | kNt, 24578);
// value codes
CGX_PIN(kFVc, 40960); CGX_PIN(kFVc | kNt, 40962);
CGX_PIN(kFVc4, 303104); CGX_PIN(kFVc4 | kNt, 303106);
CGX_PIN(kFVcPipe, 565248); CGX_PIN(kFVcPipe | kNt, 565250);
CGX_PIN(kFVc4Pipe, 827392); CGX_PIN(kFVc4Pipe | kNt, 827394);
CGX_PIN(kFVcSt, 1613824); CGX_PIN(kFVcSt | kNt, 1613826);
CGX_PIN(kFVc4St, 1875968); CGX_PIN(kFVc4St | kNt, 1875970);
CGX_PIN(kFVcMarch, 3710976); CGX_PIN(kFVcMarch | kNt, 3710978);
CGX_PIN(kFVc4March, 3973120); CGX_PIN(kFVc4March | kNt, 3973122);
CGX_PIN(kFVc4PipeT, 9216000); CGX_PIN(kFVc4PipeT | kNt, 9216002);
CGX_PIN(kFVc4StT, 10264576); CGX_PIN(kFVc4StT | kNt, 10264578);
CGX_PIN(kFVc4MarchT, 12361728); CGX_PIN(kFVc4MarchT | kNt, 12361730);
// the lean walk's request, the request masks
CGX_PIN(kVlBase, 10258434); CGX_PIN(kVL | kVlBase, 43812866);
CGX_PIN(kSellBits, 12384274); CGX_PIN(kCsrBits, 319);
// ablations
CGX_PIN(kCsrPipe | kNt | kAblG, 31); CGX_PIN(kCsrPipe | kNt | kAblR, 47);
CGX_PIN(kCsrPipe | kNt | kAblG | kAblR, 63);
CGX_PIN(kCsrPipe | kNt | kAblG | kAblR | kIL, 67108927);
CGX_PIN(kCsrPipe | kNt | kAblR | kIL, 67108911);
#undef CGX_PIN
// the lists hold what the pins name: 56 - 4 retired = 52 forms, 5 ablations
#define CGX_COUNT(VV) +1
static_assert(0 CGX_SPMV_LIST(CGX_COUNT) == 52, "k_spmv_dot forms");
static_assert(0 CGX_FD_LIST(CGX_COUNT) == 26, "k_spmv_fd forms");
static_assert(0 CGX_FUSED_LIST(CGX_COUNT) == 38, "k_spmv_fused forms");
static_assert(0 CGX_PUSH_LIST(CGX_COUNT) == 24, "k_spmv_dot_push forms");
static_assert(0 CGX_ABLATION_LIST(CGX_COUNT) == 5, "ablation forms");
#undef CGX_COUNT

}  // namespace cgx
