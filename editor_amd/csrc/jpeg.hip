// Baseline-JPEG decode for the input pipeline: what `Image.open(path).convert('RGB')` + the three
// 256-wide crops of data/datasets/bases.py:9-41 produce for the stitched tri-modal images, split the MI355X way:
//   host   (editor_jpeg_parse / editor_jpeg_entropy_decode): marker parsing and the inherently serial Huffman decode of
//          the scan(s) into quantised DCT coefficient blocks - nothing else;
//   device (editor_jpeg_reconstruct): dequantisation + 8x8 inverse DCT, chroma upsampling, YCbCr -> RGB and the crop split,
//          for a whole batch per launch, writing the uint8 (crop, B, H, cw, 3) tensors editor_resize_u8 consumes.
//          (editor_jpeg_reconstruct_ragged): the same arithmetic for a batch whose files differ in size and sampling - the
//          separate-file data sets (RGBNT201, MSVR310) - geometry from a device table, output packed image after image for
//          editor_resize_u8_ragged; still one IDCT launch and one colour launch per batch.
//          (editor_jpeg_entropy_device, with its planner editor_jpeg_plan and host twin editor_jpeg_entropy_segments): the
//          Huffman decode itself for files with one whole-frame sequential scan, one wave per restart segment of the batch, so
//          such files cross the bus as compressed bytes (DeviceJpegDecoder(entropy="device"); the host decode stays the default).
//          (editor_jpeg_entropy_split_device, host twin editor_jpeg_entropy_split_segments): the same decode, parallel INSIDE a
//          segment - 256 lanes per segment, self-synchronising subsequences - for files without restart markers
//          (DeviceJpegDecoder(entropy="device_split")).
// The arithmetic restates libjpeg's default decompression path - the one Pillow runs (JDCT_ISLOW, do_fancy_upsampling) -
// integer for integer, so the pixels are BIT-IDENTICAL to Pillow's (tests/golden/f14_decode.npz):
//   jidctint.c  jpeg_idct_islow      13-bit constants, two passes, DESCALE rounding, range-limit table
//   jdsample.c  h2v1 / h2v2 fancy    triangle filter (3/4, 1/4), edge replication at the TRUE (unpadded) plane size
//   jdcolor.c   ycc_rgb_convert      16-bit fixed-point tables, ONE_HALF folded into the Cb->G term
// Supported: 8-bit baseline / extended sequential Huffman (SOF0 / SOF1) and PROGRESSIVE Huffman (SOF2, round 4: spectral
// selection + successive approximation, jdphuff.c - the scans only refine the same quantised coefficient planes, which is all
// the device side consumes), 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, interleaved or per-component scans, restart intervals,
// JFIF (YCbCr) and Adobe transform 0 / 1.  A progressive file whose scans do not deliver every coefficient at full precision
// (truncated download) is EDITOR_JPEG_CORRUPT: libjpeg would blend neighbouring blocks there (block smoothing), which the
// device kernels do not restate.  Arithmetic-coded, lossless, 12-bit and 4-component files return EDITOR_JPEG_UNSUPPORTED
// (the caller decides; there is no silent fallback here).
#include "common.h"
#include "../../include/editor_hip.h"
#include <string.h>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// host: markers + Huffman
// ------------------------------------------------------------------------------------------------------------------
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTab {
    bool present = false;
    uint8_t bits[17]; int nvals = 0;   // the compact DHT form (what the scan planner hands to the device)
    uint8_t vals[256];
    int maxcode[18];          // largest code of each length (-1: none)
    int valoff[17];           // vals index of the first code of each length minus that code
    uint16_t look[512];       // 9-bit lookahead: (length << 8) | symbol, 0 = longer code
};

bool build_huff(HuffTab& t, const uint8_t* bits /* [1..16] */, const uint8_t* vals, int nvals)
{
    int code = 0, k = 0;
    memset(t.look, 0, sizeof(t.look));
    memcpy(t.vals, vals, nvals);
    memcpy(t.bits, bits, 17); t.nvals = nvals;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
            // (checked BEFORE anything is written: a table with more codes of a length than that length can hold - the
            //  Kraft sum libjpeg's jpeg_make_d_derived_tbl rejects - would index past look[512])
            if (k >= nvals || code >= (1 << l)) return false;
            if (l <= 9) {
                const int first = code << (9 - l);
                for (int f = 0; f < (1 << (9 - l)); ++f) t.look[first + f] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        t.maxcode[l] = bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.present = true;
    return true;
}

struct BitReader {
    const uint8_t* p; const uint8_t* end;
    uint64_t acc = 0; int nbits = 0;
    bool marker = false;          // a marker was met: the segment's data is exhausted (zeros are fed, as libjpeg does)
    void fill() {
        while (nbits <= 56) {
            uint8_t b = 0;
            if (!marker && p < end) {
                b = *p;
                if (b == 0xFF) {
                    if (p + 1 < end && p[1] == 0x00) p += 2;
                    else { marker = true; b = 0; }
                } else ++p;
            } else {
                marker = true;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    int peek(int n) { if (nbits < n) fill(); return (int)((acc >> (nbits - n)) & ((1u << n) - 1)); }
    void drop(int n) { nbits -= n; }
    int get(int n) { if (n == 0) return 0; const int v = peek(n); drop(n); return v; }
    int get1() { const int v = peek(1); drop(1); return v; }
    void restart() { acc = 0; nbits = 0; marker = false; }
};

inline int huff_decode(BitReader& br, const HuffTab& t)
{
    const int pk = br.peek(9);
    const uint16_t e = t.look[pk];
    if (e) { br.drop(e >> 8); return e & 0xff; }
    int code = br.peek(16);                           // slow path: lengths 10..16
    for (int l = 10; l <= 16; ++l) {
        const int c = code >> (16 - l);
        if (c <= t.maxcode[l]) { br.drop(l); return t.vals[(c + t.valoff[l]) & 0xff]; }
    }
    br.drop(16);
    return -1;                                        // corrupt stream
}
inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct Comp { int id, hs, vs, tq, td, ta; int bw, bh; long off; };

// What editor_jpeg_plan records at the FIRST scan header of a headers-only walk: the state a sequential scan decodes with
// (tables and restart interval as they stand THERE, not at the end of the file) and where its entropy-coded bytes begin.
enum { DHT_BYTES = 272 };                          // 16 length counts + up to 256 values
struct ScanPlan {
    int nsos = 0;
    bool whole_frame_in_order = false;             // one interleaved scan naming every component in frame order (or the lone one)
    bool tables_present = false;                   // every quantisation / Huffman table the scan names has been defined
    long ecs = 0;                                  // first entropy-coded byte
    int restart = 0;
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    uint8_t dht[8][DHT_BYTES];                     // DC tables 0..3, AC tables 0..3; only the ones the scan names are filled
};

struct Jpeg {
    int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
    Comp comp[3];
    uint16_t qt[4][64]; bool qt_ok[4] = {false, false, false, false};
    HuffTab dc[4], ac[4];
    int restart = 0;
    bool progressive = false, unsupported = false, have_sof = false;
    int adobe_transform = -1; bool jfif = false;
    long total_blocks = 0;
    bool covered[3] = {false, false, false};      // components some scan has delivered
    int8_t coef_al[3][64];                        // progressive: successive-approximation bit each coefficient has reached (-1: none yet)
    ScanPlan* plan = nullptr;                     // headers-only walks of editor_jpeg_plan
};

void dht_compact(const HuffTab& t, uint8_t* out)
{
    memset(out, 0, DHT_BYTES);
    if (!t.present) return;
    memcpy(out, t.bits + 1, 16);
    memcpy(out + 16, t.vals, t.nvals);
}

void record_scan(const Jpeg& j, int ns, const int* idx, long ecs)
{
    ScanPlan& p = *j.plan;
    if (++p.nsos != 1) return;
    p.ecs = ecs; p.restart = j.restart;
    p.whole_frame_in_order = ns == j.ncomp;
    p.tables_present = true;
    memset(p.dht, 0, sizeof(p.dht));
    for (int i = 0; i < ns; ++i) {
        const Comp& k = j.comp[idx[i]];
        if (idx[i] != i) p.whole_frame_in_order = false;
        if (!j.qt_ok[k.tq] || !j.dc[k.td].present || !j.ac[k.ta].present) p.tables_present = false;
        if (idx[i] == i) { p.td[i] = k.td; p.ta[i] = k.ta; }
        dht_compact(j.dc[k.td], p.dht[k.td]);
        dht_compact(j.ac[k.ta], p.dht[4 + k.ta]);
    }
}

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parses the markers up to (and including the header of) each SOS.  `coef` NULL: headers only; otherwise `coef` holds
// `coef_blocks` blocks of 64 coefficients and every scan is checked against that size before it writes.
int decode(const uint8_t* d, long n, Jpeg& j, int16_t* coef, long coef_blocks)
{
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return EDITOR_JPEG_CORRUPT;
    long pos = 2;
    bool seen_scan = false;
    while (pos + 4 <= n) {
        if (d[pos] != 0xFF) { ++pos; continue; }
        const int m = d[pos + 1];
        if (m == 0xFF) { ++pos; continue; }
        if (m == 0xD9) break;                                             // EOI
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }
        const long len = rd16(d + pos + 2);
        if (len < 2 || pos + 2 + len > n) return EDITOR_JPEG_CORRUPT;
        const uint8_t* s = d + pos + 4;
        const long sl = len - 2;
        if (m == 0xDB) {                                                  // DQT
            long o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (tq > 3) return EDITOR_JPEG_CORRUPT;
                ++o;
                if (o + (pq ? 128 : 64) > sl) return EDITOR_JPEG_CORRUPT;
                for (int i = 0; i < 64; ++i) {
                    j.qt[tq][kZigzag[i]] = pq ? (uint16_t)rd16(s + o + 2 * i) : s[o + i];
                }
                o += pq ? 128 : 64;
                j.qt_ok[tq] = true;
            }
        } else if (m == 0xC4) {                                           // DHT
            long o = 0;
            while (o + 17 <= sl) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return EDITOR_JPEG_CORRUPT;
                uint8_t bits[17]; bits[0] = 0;
                int cnt = 0;
                for (int i = 1; i <= 16; ++i) { bits[i] = s[o + i]; cnt += bits[i]; }
                if (cnt > 256 || o + 17 + cnt > sl) return EDITOR_JPEG_CORRUPT;
                if (!build_huff(tc ? j.ac[th] : j.dc[th], bits, s + o + 17, cnt)) return EDITOR_JPEG_CORRUPT;
                o += 17 + cnt;
            }
        } else if (m == 0xC0 || m == 0xC1 || m == 0xC2 || (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            if (m != 0xC0 && m != 0xC1 && m != 0xC2) { j.unsupported = true; return EDITOR_JPEG_UNSUPPORTED; }   // lossless / arithmetic / hierarchical
            j.progressive = m == 0xC2;
            memset(j.coef_al, -1, sizeof(j.coef_al));
            if (j.have_sof) return EDITOR_JPEG_CORRUPT;                   // one frame per file (a second SOF would re-size the block grid under the scans)
            if (sl < 6 || s[0] != 8) { j.unsupported = true; return EDITOR_JPEG_UNSUPPORTED; }
            j.H = rd16(s + 1); j.W = rd16(s + 3); j.ncomp = s[5];
            if ((j.ncomp != 1 && j.ncomp != 3) || j.W <= 0 || j.H <= 0 || sl < 6 + 3 * j.ncomp) return EDITOR_JPEG_UNSUPPORTED;
            for (int c = 0; c < j.ncomp; ++c) {
                Comp& k = j.comp[c];
                k.id = s[6 + 3 * c]; k.hs = s[7 + 3 * c] >> 4; k.vs = s[7 + 3 * c] & 15; k.tq = s[8 + 3 * c];
                if (k.hs < 1 || k.vs < 1 || k.tq > 3) return EDITOR_JPEG_CORRUPT;
                j.hmax = k.hs > j.hmax ? k.hs : j.hmax; j.vmax = k.vs > j.vmax ? k.vs : j.vmax;
            }
            if (j.ncomp == 1) { j.comp[0].hs = j.comp[0].vs = 1; j.hmax = j.vmax = 1; }      // (a lone component is never subsampled)
            else {
                // luma carries the full resolution, both chroma planes share one of 1x1 / (hmax)x(vmax) reductions
                if (j.comp[0].hs != j.hmax || j.comp[0].vs != j.vmax || j.comp[1].hs != 1 || j.comp[1].vs != 1 ||
                    j.comp[2].hs != 1 || j.comp[2].vs != 1 || j.hmax > 2 || j.vmax > 2 || (j.hmax == 1 && j.vmax == 2))
                    return EDITOR_JPEG_UNSUPPORTED;
            }
            j.mcux = (j.W + 8 * j.hmax - 1) / (8 * j.hmax); j.mcuy = (j.H + 8 * j.vmax - 1) / (8 * j.vmax);
            long off = 0;
            for (int c = 0; c < j.ncomp; ++c) {
                Comp& k = j.comp[c];
                k.bw = j.mcux * k.hs; k.bh = j.mcuy * k.vs; k.off = off;
                off += (long)k.bw * k.bh;
            }
            j.total_blocks = off;
            j.have_sof = true;
        } else if (m == 0xDD) {
            if (sl < 2) return EDITOR_JPEG_CORRUPT;
            j.restart = rd16(s);
        } else if (m == 0xE0 && sl >= 5 && !memcmp(s, "JFIF", 5)) {
            j.jfif = true;
        } else if (m == 0xEE && sl >= 12 && !memcmp(s, "Adobe", 5)) {
            j.adobe_transform = s[11];
        } else if (m == 0xDA) {                                           // SOS
            if (!j.have_sof || sl < 1) return EDITOR_JPEG_CORRUPT;
            const int ns = s[0];
            if (ns < 1 || ns > j.ncomp || sl < 1 + 2 * ns + 3) return EDITOR_JPEG_CORRUPT;
            int idx[3];
            for (int i = 0; i < ns; ++i) {
                int c = -1;
                for (int q = 0; q < j.ncomp; ++q) if (j.comp[q].id == s[1 + 2 * i]) c = q;
                if (c < 0) return EDITOR_JPEG_CORRUPT;
                idx[i] = c; j.comp[c].td = s[2 + 2 * i] >> 4; j.comp[c].ta = s[2 + 2 * i] & 15;
                if (j.comp[c].td > 3 || j.comp[c].ta > 3) return EDITOR_JPEG_CORRUPT;
            }
            pos += 2 + len;
            seen_scan = true;
            if (!coef) {                                                  // headers only: skip the entropy-coded segment
                if (j.plan) record_scan(j, ns, idx, pos);
                while (pos + 1 < n && !(d[pos] == 0xFF && d[pos + 1] != 0x00 && !(d[pos + 1] >= 0xD0 && d[pos + 1] <= 0xD7))) ++pos;
                continue;
            }
            if (j.total_blocks > coef_blocks) return EDITOR_JPEG_CORRUPT;  // (the frame this scan belongs to must fit the caller's buffer)
            // scan parameters (B.2.3): spectral selection Ss..Se, successive approximation Ah / Al - sequential scans carry 0,63,0,0
            const uint8_t* sp = s + 1 + 2 * ns;
            const int Ss = sp[0], Se = sp[1], Ah = sp[2] >> 4, Al = sp[2] & 15;
            const bool prog = j.progressive;
            if (prog) {
                // jdphuff.c start_pass_phuff_decoder's validity rules
                if (Ss > Se || Se > 63 || Al > 13 || (Ah != 0 && Al != Ah - 1)) return EDITOR_JPEG_CORRUPT;
                if (Ss == 0 ? Se != 0 : ns != 1) return EDITOR_JPEG_CORRUPT;
            }
            for (int i = 0; i < ns; ++i) {
                const Comp& k = j.comp[idx[i]];
                if (!j.qt_ok[k.tq]) return EDITOR_JPEG_CORRUPT;
                if (!prog) {
                    if (!j.dc[k.td].present || !j.ac[k.ta].present) return EDITOR_JPEG_CORRUPT;
                    if (j.covered[idx[i]]) return EDITOR_JPEG_CORRUPT;      // sequential coding: one scan per component
                    j.covered[idx[i]] = true;
                } else {
                    if (Ss == 0 && Ah == 0 && !j.dc[k.td].present) return EDITOR_JPEG_CORRUPT;
                    if (Ss > 0 && !j.ac[k.ta].present) return EDITOR_JPEG_CORRUPT;
                    // a refinement scan refines what a first scan delivered at exactly the bit above; a first scan delivers
                    // coefficients nobody has delivered yet (libjpeg only warns; such files are not decodable unambiguously)
                    for (int kk = Ss; kk <= Se; ++kk) {
                        if (j.coef_al[idx[i]][kk] != (Ah == 0 ? -1 : Ah)) return EDITOR_JPEG_CORRUPT;
                        j.coef_al[idx[i]][kk] = (int8_t)Al;
                    }
                }
            }
            BitReader br{d + pos, d + n};
            int pred[3] = {0, 0, 0};
            int eobrun = 0;                                               // progressive AC scans: blocks still covered by an end-of-band run
            // MCU geometry of this scan: interleaved -> hs x vs blocks per component per MCU over mcux x mcuy MCUs;
            // a single-component scan -> one block per MCU over the component's own (unpadded) block grid
            int nx = j.mcux, ny = j.mcuy;
            if (ns == 1) {
                const Comp& k = j.comp[idx[0]];
                nx = ((j.W * k.hs + j.hmax - 1) / j.hmax + 7) / 8;
                ny = ((j.H * k.vs + j.vmax - 1) / j.vmax + 7) / 8;
            }
            int left = j.restart, rst = 0;
            for (int my = 0; my < ny; ++my)
                for (int mx = 0; mx < nx; ++mx) {
                    if (j.restart && left == 0) {
                        // byte-align, expect RSTn
                        br.restart();
                        const uint8_t* q = br.p;
                        while (q + 1 < br.end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) {
                            if (q[0] == 0xFF && q[1] != 0x00 && q[1] != 0xFF) break;      // some other marker: give up on resync
                            ++q;
                        }
                        if (q + 1 < br.end && q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7) q += 2;
                        br.p = q;
                        (void)rst; ++rst;
                        pred[0] = pred[1] = pred[2] = 0;
                        eobrun = 0;
                        left = j.restart;
                    }
                    for (int i = 0; i < ns; ++i) {
                        const Comp& k = j.comp[idx[i]];
                        const int bh_ = ns == 1 ? 1 : k.vs, bw_ = ns == 1 ? 1 : k.hs;
                        for (int by = 0; by < bh_; ++by)
                            for (int bx = 0; bx < bw_; ++bx) {
                                const int gx = mx * bw_ + bx, gy = my * bh_ + by;
                                int16_t* blk = coef + (k.off + (long)gy * k.bw + gx) * 64;
                                if (!prog) {
                                    memset(blk, 0, 128);
                                    const int sdc = huff_decode(br, j.dc[k.td]);
                                    if (sdc < 0 || sdc > 11) return EDITOR_JPEG_CORRUPT;
                                    const int diff = sdc ? extend(br.get(sdc), sdc) : 0;
                                    pred[idx[i]] += diff;
                                    blk[0] = (int16_t)pred[idx[i]];
                                    for (int kk = 1; kk < 64;) {
                                        const int rs = huff_decode(br, j.ac[k.ta]);
                                        if (rs < 0) return EDITOR_JPEG_CORRUPT;
                                        const int r = rs >> 4, sz = rs & 15;
                                        if (sz == 0) { if (r == 15) { kk += 16; continue; } break; }
                                        kk += r;
                                        if (kk > 63) return EDITOR_JPEG_CORRUPT;
                                        blk[kZigzag[kk]] = (int16_t)extend(br.get(sz), sz);
                                        ++kk;
                                    }
                                } else if (Ss == 0) {
                                    if (Ah == 0) {                        // decode_mcu_DC_first: the DC difference, scaled by 2^Al
                                        const int sdc = huff_decode(br, j.dc[k.td]);
                                        if (sdc < 0 || sdc > 11) return EDITOR_JPEG_CORRUPT;
                                        const int diff = sdc ? extend(br.get(sdc), sdc) : 0;
                                        pred[idx[i]] += diff;
                                        blk[0] = (int16_t)(pred[idx[i]] * (1 << Al));
                                    } else if (br.get1()) {               // decode_mcu_DC_refine: one more bit of every DC value
                                        blk[0] = (int16_t)(blk[0] | (1 << Al));
                                    }
                                } else if (Ah == 0) {                     // decode_mcu_AC_first
                                    if (eobrun > 0) { --eobrun; continue; }
                                    for (int kk = Ss; kk <= Se; ++kk) {
                                        const int rs = huff_decode(br, j.ac[k.ta]);
                                        if (rs < 0) return EDITOR_JPEG_CORRUPT;
                                        const int r = rs >> 4, sz = rs & 15;
                                        if (sz) {
                                            kk += r;
                                            if (kk > 63) return EDITOR_JPEG_CORRUPT;
                                            blk[kZigzag[kk]] = (int16_t)(extend(br.get(sz), sz) * (1 << Al));
                                        } else if (r == 15) {
                                            kk += 15;                      // ZRL: sixteen zeros
                                        } else {                           // EOBr: this block and the next 2^r + bits - 1 end here
                                            eobrun = (1 << r) - 1;
                                            if (r) eobrun += br.get(r);
                                            break;
                                        }
                                    }
                                } else {                                  // decode_mcu_AC_refine
                                    const int p1 = 1 << Al, m1 = -(1 << Al);
                                    int kk = Ss;
                                    if (eobrun == 0) {
                                        for (; kk <= Se; ++kk) {
                                            const int rs = huff_decode(br, j.ac[k.ta]);
                                            if (rs < 0) return EDITOR_JPEG_CORRUPT;
                                            int r = rs >> 4, sv = rs & 15;
                                            if (sv) {
                                                if (sv != 1) return EDITOR_JPEG_CORRUPT;     // (libjpeg warns and goes on with size 1)
                                                sv = br.get1() ? p1 : m1;
                                            } else if (r != 15) {
                                                eobrun = 1 << r;           // EOBr: the run includes this block, whose remaining
                                                if (r) eobrun += br.get(r);  // non-zero coefficients still get their correction bits
                                                break;
                                            }
                                            // skip r still-zero coefficients, refining every already non-zero one on the way
                                            do {
                                                int16_t* c = blk + kZigzag[kk];
                                                if (*c != 0) {
                                                    if (br.get1() && (*c & p1) == 0) *c = (int16_t)(*c + (*c >= 0 ? p1 : m1));
                                                } else if (--r < 0) {
                                                    break;
                                                }
                                                ++kk;
                                            } while (kk <= Se);
                                            if (sv) {
                                                if (kk > 63) return EDITOR_JPEG_CORRUPT;
                                                blk[kZigzag[kk]] = (int16_t)sv;
                                            }
                                        }
                                    }
                                    if (eobrun > 0) {
                                        for (; kk <= Se; ++kk) {
                                            int16_t* c = blk + kZigzag[kk];
                                            if (*c != 0 && br.get1() && (*c & p1) == 0) *c = (int16_t)(*c + (*c >= 0 ? p1 : m1));
                                        }
                                        --eobrun;
                                    }
                                }
                            }
                    }
                    if (j.restart) --left;
                }
            // continue the marker scan after the entropy-coded data
            pos = br.p - d;
            while (pos + 1 < n && !(d[pos] == 0xFF && d[pos + 1] != 0x00 && !(d[pos + 1] >= 0xD0 && d[pos + 1] <= 0xD7))) ++pos;
            continue;
        }
        pos += 2 + len;
    }
    if (!j.have_sof || !seen_scan) return EDITOR_JPEG_CORRUPT;
    if (coef)                                                             // every component delivered by some scan, or the planes
        for (int c = 0; c < j.ncomp; ++c) {                               // of the missing ones would be whatever the buffer held
            if (!j.progressive) { if (!j.covered[c]) return EDITOR_JPEG_CORRUPT; continue; }
            // progressive: every coefficient at full precision (an incomplete file is where libjpeg would smooth blocks)
            for (int kk = 0; kk < 64; ++kk) if (j.coef_al[c][kk] != 0) return EDITOR_JPEG_CORRUPT;
        }
    return 0;
}

void fill_info(const Jpeg& j, int* info)
{
    info[0] = j.W; info[1] = j.H; info[2] = j.ncomp; info[3] = j.hmax; info[4] = j.vmax; info[5] = j.mcux; info[6] = j.mcuy;
    // colour transform of the decompressor's default choice (jdapimin.c default_decompress_parms): 1 = YCbCr -> RGB
    int tr = 0;
    if (j.ncomp == 3) {
        if (j.jfif) tr = 1;
        else if (j.adobe_transform >= 0) tr = j.adobe_transform == 1 ? 1 : 0;
        else tr = !(j.comp[0].id == 'R' && j.comp[1].id == 'G' && j.comp[2].id == 'B');
    }
    info[7] = tr;
    info[8] = (int)j.total_blocks;
    for (int c = 0; c < 3; ++c) { info[9 + c] = c < j.ncomp ? j.comp[c].tq : 0; }
}

// ------------------------------------------------------------------------------------------------------------------
// device: reconstruction
// ------------------------------------------------------------------------------------------------------------------
struct JpegGeom {
    int W, H, ncomp, hmax, vmax, mcux, mcuy, transform;
    int bw[3], bh[3]; long off[3];          // block grids (padded to whole MCUs) and first block of each component
    long blocks_per_image;
    long plane_off[3]; int pw[3], ph[3];    // sample planes (padded): pw = 8 bw, ph = 8 bh; byte offsets inside one image's planes
    long plane_bytes;
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// jpeg_idct_islow's output map: sample_range_limit + CENTERJSAMPLE indexed by (x & RANGE_MASK), RANGE_MASK = 1023
__device__ __forceinline__ uint8_t range_limit_centered(int x)
{
    const int i = x & 1023;
    return (uint8_t)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// one 1-D pass of jidctint.c (CONST_BITS 13): in[8] -> out[8] before the final DESCALE (shift given by the caller)
__device__ __forceinline__ void idct_1d(const int (&in)[8], int (&out)[8], int shift)
{
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * FIX_0_541196100;
    int tmp2 = z1 + z3 * (-FIX_1_847759065);
    int tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = in[0]; z3 = in[4];
    int tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 *= FIX_0_298631336; tmp1 *= FIX_2_053119869; tmp2 *= FIX_3_072711026; tmp3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = descale(tmp10 + tmp3, shift); out[7] = descale(tmp10 - tmp3, shift);
    out[1] = descale(tmp11 + tmp2, shift); out[6] = descale(tmp11 - tmp2, shift);
    out[2] = descale(tmp12 + tmp1, shift); out[5] = descale(tmp12 - tmp1, shift);
    out[3] = descale(tmp13 + tmp0, shift); out[4] = descale(tmp13 - tmp0, shift);
}

// one 8x8 block: dequantise, columns (-> scaled by 2^PASS1_BITS), rows, range limit, 8 rows of 8 bytes at dst (row pitch pw;
// dst 8-byte aligned: uint2 stores)
__device__ __forceinline__ void idct_block(const int16_t* __restrict__ in, const uint16_t* __restrict__ q, uint8_t* __restrict__ dst, int pw)
{
    int ws[8][8];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int v[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = (int)in[r * 8 + col] * (int)q[r * 8 + col];
        idct_1d(v, o, 13 - 2);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][col] = o[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int o[8];
        idct_1d(ws[r], o, 13 + 2 + 3);
        uint2 pk;
        pk.x = range_limit_centered(o[0]) | (range_limit_centered(o[1]) << 8) | (range_limit_centered(o[2]) << 16) | ((uint32_t)range_limit_centered(o[3]) << 24);
        pk.y = range_limit_centered(o[4]) | (range_limit_centered(o[5]) << 8) | (range_limit_centered(o[6]) << 16) | ((uint32_t)range_limit_centered(o[7]) << 24);
        *reinterpret_cast<uint2*>(dst + (long)r * pw) = pk;
    }
}

template <typename T> __device__ __forceinline__ T pick3(const T (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// block `bi` of one image (coefficients at `in`, its three quantisation tables at `q3`) -> its place in the image's planes `pl`
__device__ __forceinline__ void idct_image_block(const int16_t* __restrict__ in, const uint16_t* __restrict__ q3, const JpegGeom& g, long bi,
                                                 uint8_t* __restrict__ pl)
{
    const int c = (g.ncomp > 1 && bi >= g.off[1]) ? (bi >= g.off[2] ? 2 : 1) : 0;
    // (selects, not g.x[c]: a geometry built in registers by the ragged kernel would go to scratch under a dynamic index)
    const long lb = bi - pick3(g.off, c);
    const int bw = pick3(g.bw, c), pw = pick3(g.pw, c);
    const int by = (int)(lb / bw), bx = (int)(lb % bw);
    idct_block(in, q3 + c * 64, pl + pick3(g.plane_off, c) + ((long)by * 8) * pw + bx * 8, pw);
}

// one thread per 8x8 block of a batch of ONE geometry
__global__ __launch_bounds__(128) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, JpegGeom g, int B,
                                                        uint8_t* __restrict__ planes)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * g.blocks_per_image) return;
    const int img = (int)(t / g.blocks_per_image);
    const long bi = t % g.blocks_per_image;
    idct_image_block(coef + t * 64, qt + (long)img * 3 * 64, g, bi, planes + (long)img * g.plane_bytes);
}

__device__ __forceinline__ int clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// chroma sample at full-resolution pixel (x, y) by jdsample.c's fancy upsampling (or the plain value for 1x1)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pw, int cw, int ch, int hmax, int vmax, int x, int y)
{
    if (hmax == 1) return p[(long)y * pw + x];                          // 4:4:4
    const int cx = x >> 1, right = x & 1;
    if (vmax == 1) {                                                    // h2v1_fancy_upsample
        const uint8_t* r = p + (long)y * pw;
        const int v = r[cx];
        if (right) return cx == cw - 1 ? v : (3 * v + r[cx + 1] + 2) >> 2;
        return cx == 0 ? v : (3 * v + r[cx - 1] + 1) >> 2;
    }
    // h2v2_fancy_upsample: nearer row 3/4, further row 1/4 (context rows replicate at the top / bottom of the TRUE plane)
    const int cy = y >> 1, lower = y & 1;
    int oy = lower ? cy + 1 : cy - 1;
    oy = oy < 0 ? 0 : (oy > ch - 1 ? ch - 1 : oy);
    const uint8_t* r0 = p + (long)cy * pw;
    const uint8_t* r1 = p + (long)oy * pw;
    const int thiscol = 3 * r0[cx] + r1[cx];
    if (right) {
        if (cx == cw - 1) return (thiscol * 4 + 7) >> 4;
        return (thiscol * 3 + (3 * r0[cx + 1] + r1[cx + 1]) + 7) >> 4;
    }
    if (cx == 0) return (thiscol * 4 + 8) >> 4;
    return (thiscol * 3 + (3 * r0[cx - 1] + r1[cx - 1]) + 8) >> 4;
}

// pixel (x, y) of one image from its planes `pl`: (upsampled) Y, Cb, Cr -> RGB (jdcolor.c ycc_rgb_convert); a lone component
// is replicated (`convert('RGB')` of a grayscale file)
__device__ __forceinline__ void color_pixel(const uint8_t* __restrict__ pl, const JpegGeom& g, int x, int y, uint8_t* __restrict__ o)
{
    const int yv = pl[g.plane_off[0] + (long)y * g.pw[0] + x];
    int r = yv, gg = yv, b = yv;
    if (g.ncomp == 3) {
        const int cw = (g.W + g.hmax - 1) / g.hmax, ch = (g.H + g.vmax - 1) / g.vmax;      // true downsampled size
        const int cb = chroma_at(pl + g.plane_off[1], g.pw[1], cw, ch, g.hmax, g.vmax, x, y);
        const int cr = chroma_at(pl + g.plane_off[2], g.pw[2], cw, ch, g.hmax, g.vmax, x, y);
        if (g.transform) {
            const int xb = cb - 128, xr = cr - 128;
            r = clamp255(yv + ((91881 * xr + 32768) >> 16));
            b = clamp255(yv + ((116130 * xb + 32768) >> 16));
            gg = clamp255(yv + ((-22554 * xb + 32768 - 46802 * xr) >> 16));
        } else {
            r = yv; gg = cb; b = cr;
        }
    }
    o[0] = (uint8_t)r; o[1] = (uint8_t)gg; o[2] = (uint8_t)b;
}

// one thread per output pixel, written into crop x / crop_w of out (ncrop, B, H, crop_w, 3); pixels right of the last whole
// crop are dropped (bases.py:19-21: range(W // 256))
__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ planes, JpegGeom g, int B, int crop_w, int ncrop,
                                                         uint8_t* __restrict__ out)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int wuse = crop_w * ncrop;
    if (t >= (long)B * g.H * wuse) return;
    const int x = (int)(t % wuse), y = (int)((t / wuse) % g.H), img = (int)(t / ((long)wuse * g.H));
    const int crop = x / crop_w, xc = x % crop_w;
    color_pixel(planes + (long)img * g.plane_bytes, g, x, y, out + ((((long)crop * B + img) * g.H + y) * crop_w + xc) * 3);
}

__host__ __device__ inline bool make_geom(const int* info, JpegGeom& g)
{
    g.W = info[0]; g.H = info[1]; g.ncomp = info[2]; g.hmax = info[3]; g.vmax = info[4]; g.mcux = info[5]; g.mcuy = info[6];
    g.transform = info[7];
    if ((g.ncomp != 1 && g.ncomp != 3) || g.W <= 0 || g.H <= 0 || g.mcux <= 0 || g.mcuy <= 0) return false;
    long off = 0, poff = 0;
    for (int c = 0; c < 3; ++c) {
        const int hs = c == 0 ? g.hmax : 1, vs = c == 0 ? g.vmax : 1;
        g.bw[c] = c < g.ncomp ? g.mcux * hs : 0; g.bh[c] = c < g.ncomp ? g.mcuy * vs : 0;
        g.off[c] = off; off += (long)g.bw[c] * g.bh[c];
        g.pw[c] = g.bw[c] * 8; g.ph[c] = g.bh[c] * 8;
        g.plane_off[c] = poff; poff += (long)g.pw[c] * g.ph[c];
    }
    if (g.ncomp == 1) { g.off[1] = g.off[2] = off; }
    g.blocks_per_image = off;
    g.plane_bytes = poff;
    return off == info[8];
}

// ---- ragged batch: every image its own geometry ---------------------------------------------------------------------
// info: (B,16) int32 rows of editor_jpeg_parse; tab: (5,B) int64 = first coefficient block, plane byte offset (8-byte
// aligned: uint2 stores), output byte offset, inclusive prefix sum of blocks, inclusive prefix sum of output pixels.
enum { RT_COEF = 0, RT_PLANE = 1, RT_OUT = 2, RT_BLOCKS = 3, RT_PIXELS = 4, RT_ROWS = 5 };

__global__ __launch_bounds__(128) void jpeg_idct_ragged_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt,
                                                               const int* __restrict__ info, const long* __restrict__ tab, int B, long nblocks,
                                                               uint8_t* __restrict__ planes)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nblocks) return;
    const long* prefix = tab + (long)RT_BLOCKS * B;
    const int img = ragged_find(prefix, B, t);
    const long bi = t - (img ? prefix[img - 1] : 0);
    JpegGeom g;
    make_geom(info + (long)img * 16, g);                               // (validated on the host before the launch)
    idct_image_block(coef + (tab[(long)RT_COEF * B + img] + bi) * 64, qt + (long)img * 3 * 64, g, bi, planes + tab[(long)RT_PLANE * B + img]);
}

// one thread per output pixel of the packed output: image i is (H_i, W_i, 3) row-major at its output offset (no crop split)
__global__ __launch_bounds__(256) void jpeg_color_ragged_kernel(const uint8_t* __restrict__ planes, const int* __restrict__ info,
                                                                const long* __restrict__ tab, int B, long npixels, uint8_t* __restrict__ out)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npixels) return;
    const long* prefix = tab + (long)RT_PIXELS * B;
    const int img = ragged_find(prefix, B, t);
    const long p = t - (img ? prefix[img - 1] : 0);
    JpegGeom g;
    make_geom(info + (long)img * 16, g);
    color_pixel(planes + tab[(long)RT_PLANE * B + img], g, (int)(p % g.W), (int)(p / g.W), out + tab[(long)RT_OUT * B + img] + p * 3);
}


// ------------------------------------------------------------------------------------------------------------------
// sequential-scan entropy decode, one restart segment at a time: ONE routine for the host twin and the device kernel
// ------------------------------------------------------------------------------------------------------------------
// A device-eligible file (editor_jpeg_plan) has one interleaved scan whose restart markers split it into segments that
// decode independently: the DC predictors and the bit reader start afresh at each.  decode() walks such a scan MCU by MCU
// and resynchronises at every RSTn; for a scan with exactly the expected markers that is the same as decoding every
// segment on its own between the planner's byte ranges, which is what happens here.
//   bytes    every read is bounded by the segment's end (and by what the caller has staged); past it, zeros are fed
//   writes   the destination block is computed from the block's index in the segment and the geometry - never from data
//   loops    block loop: counted from the geometry; coefficient loop: index strictly increases to 64
// (the kernel's copy of kZigzag; it keeps it in LDS - a load from here per coefficient would sit on the walking lane's critical path)
__device__ __attribute__((unused)) const uint8_t kZigzagDev[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// The decoder's view of one Huffman table, derived from the compact DHT form (HuffTab without the host-only fields).
struct HuffLut {
    uint16_t look[512];       // 9-bit lookahead: (length << 8) | symbol, 0 = longer code
    int maxcode[18];
    int valoff[18];
    uint8_t vals[256];
};

// first: the per-length rows (one caller per table) ...
__host__ __device__ inline void lut_lengths(HuffLut& t, const uint8_t* dht)
{
    int code = 0, k = 0;
    t.maxcode[0] = -1; t.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int nb = dht[l - 1];
        t.valoff[l] = k - code;
        code += nb; k += nb;
        t.maxcode[l] = nb ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff; t.valoff[17] = 0;
}
// ... then, with those visible, the values and the lookahead entries, `nlanes` callers striding over them.  Entry p is the
// canonical decode of its own 9 bits, which is what build_huff's fill leaves there for a table that passed its check (the
// planner ran it); the value index is masked, so a table that did not cannot be read out of range either.
__host__ __device__ inline void lut_fill(HuffLut& t, const uint8_t* dht, int lane, int nlanes)
{
    for (int i = lane; i < 256; i += nlanes) t.vals[i] = dht[16 + i];
    for (int p = lane; p < 512; p += nlanes) {
        int e = 0;
        for (int l = 1; l <= 9; ++l) {
            const int c = p >> (9 - l);
            if (c <= t.maxcode[l]) { e = (l << 8) | dht[16 + ((c + t.valoff[l]) & 0xff)]; break; }
        }
        t.look[p] = (uint16_t)e;
    }
}

// BitReader over a WINDOW of the stream: buf[0] is stream byte `base`, bytes [base, lim) are present.  The host hands the
// whole stream (base 0, lim = its length); the kernels restage the window (SEG_MARGIN, SPLIT_MARGIN).
// TRACK: the reader can also say where it is - which loaded bytes took two stream bytes (`stuffed`, newest in bit 0) and how
// many of the loaded bits are the zeros fed past the data (`vbits`, always the newest).  Without it those two members and
// every statement that keeps them do not exist.
template <bool TRACK> struct ReaderTrack {};
template <> struct ReaderTrack<true> { int vbits; uint32_t stuffed; };
template <bool TRACK>
struct WinReader : ReaderTrack<TRACK> {
    const uint8_t* buf; long base, lim;
    long p, end;                                   // next byte; end of the segment
    uint64_t acc; int nbits; bool marker;
    // Feeds the bytes BitReader::fill feeds, in the same order; only how far ahead it reads differs (25 to 56 bits, enough
    // for any peek), which no decoded value depends on.  Four bytes at once where none of them is 0xFF: the four reads are
    // independent, the byte-by-byte path below waits for each before it knows where the next one is.
    __host__ __device__ __forceinline__ void fill() {
        while (nbits <= 24) {
            if (!marker && p >= base && p + 4 <= end && p + 4 <= lim) {
                const uint8_t* q = buf + (p - base);
                const uint32_t b0 = q[0], b1 = q[1], b2 = q[2], b3 = q[3];
                if (b0 != 0xFF && b1 != 0xFF && b2 != 0xFF && b3 != 0xFF) {
                    acc = (acc << 32) | ((b0 << 24) | (b1 << 16) | (b2 << 8) | b3);
                    nbits += 32; p += 4;
                    if constexpr (TRACK) this->stuffed <<= 4;
                    continue;
                }
            }
            uint8_t b = 0;
            if (!marker && p < end && p >= base && p < lim) {
                b = buf[p - base];
                if (b == 0xFF) {
                    if (p + 1 < end && p + 1 < lim && buf[p + 1 - base] == 0x00) { p += 2; if constexpr (TRACK) this->stuffed = (this->stuffed << 1) | 1u; }
                    else { marker = true; b = 0; }
                } else { ++p; if constexpr (TRACK) this->stuffed <<= 1; }
            } else {
                marker = true;
            }
            if constexpr (TRACK) { if (marker && this->vbits < 64) this->vbits += 8; }   // (64 or more: everything held is past the data)
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    __host__ __device__ __forceinline__ int peek(int n) { if (nbits < n) fill(); return (int)((acc >> (nbits - n)) & ((1u << n) - 1)); }
    __host__ __device__ __forceinline__ void drop(int n) { nbits -= n; }
    __host__ __device__ __forceinline__ int get(int n) { if (n == 0) return 0; const int v = peek(n); drop(n); return v; }
    // ---- TRACK only ----
    __host__ __device__ __forceinline__ void seek(long at, int bit) {
        p = at; acc = 0; nbits = 0; this->vbits = 0; this->stuffed = 0; marker = false;
        if (bit) { peek(bit); drop(bit); }
    }
    // all data consumed and the reader has met its end (call after fill())
    __host__ __device__ __forceinline__ bool exhausted() const { return marker && nbits <= this->vbits; }
    // the stream position of the next unconsumed bit: the bytes still held are walked back over, a stuffed one counting two
    __host__ __device__ __forceinline__ void cursor(long& cp, int& cbit) const {
        const int real = nbits - this->vbits;
        if (real <= 0) { cp = p; cbit = 0; return; }
        const int part = real & 7, cnt = (real + 7) >> 3;                     // (cnt <= 7: at most 56 bits are held)
        cp = p - cnt - __builtin_popcount(this->stuffed & ((1u << cnt) - 1u));
        cbit = part ? 8 - part : 0;
    }
};
using SegReader = WinReader<false>;
using SubReader = WinReader<true>;

// one Huffman symbol from either reader: the 9-bit lookahead, then the per-length rows; -1 = no such code
template <class R>
__host__ __device__ __forceinline__ int huff_symbol(R& br, const HuffLut& t)
{
    const int e = t.look[br.peek(9)];
    if (e) { br.drop(e >> 8); return e & 0xff; }
    const int code = br.peek(16);
    for (int l = 10; l <= 16; ++l) {
        const int c = code >> (16 - l);
        if (c <= t.maxcode[l]) { br.drop(l); return t.vals[(c + t.valoff[l]) & 0xff]; }
    }
    br.drop(16);
    return -1;
}
__host__ __device__ __forceinline__ int seg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Geometry of a device-eligible scan (decode()'s accepted layouts: luma hmax x vmax blocks per MCU, chroma 1 x 1).
struct ScanGeom {
    int ncomp, hmax, vmax, mcux, mcuy, restart;
    int hv, bpm;                                   // luma blocks per MCU; blocks per MCU
    long nmcu, total_blocks, off1, off2;
};
__host__ __device__ inline bool make_scan_geom(const int* fd, ScanGeom& g)
{
    g.ncomp = fd[0]; g.hmax = fd[1]; g.vmax = fd[2]; g.mcux = fd[3]; g.mcuy = fd[4]; g.restart = fd[5];
    if ((g.ncomp != 1 && g.ncomp != 3) || g.hmax < 1 || g.hmax > 2 || g.vmax < 1 || g.vmax > 2 || (g.hmax == 1 && g.vmax == 2) ||
        (g.ncomp == 1 && g.hmax * g.vmax != 1) || g.mcux < 1 || g.mcux > 8192 || g.mcuy < 1 || g.mcuy > 8192 || g.restart < 0 || g.restart > 65535)
        return false;
    g.hv = g.hmax * g.vmax; g.bpm = g.ncomp == 3 ? g.hv + 2 : 1;
    g.nmcu = (long)g.mcux * g.mcuy;
    g.off1 = g.nmcu * g.hv; g.off2 = g.off1 + g.nmcu;
    g.total_blocks = g.ncomp == 3 ? g.off2 + g.nmcu : g.nmcu;
    return true;
}
// block `b` (MCU-major, as the scan delivers them) of the segment whose first MCU is m0 -> its block in the image and its
// component.  m0 * bpm + b < nmcu * bpm (the callers' loop bound) puts the result inside [0, total_blocks).
__host__ __device__ __forceinline__ long scan_block(const ScanGeom& g, long m0, long b, int& c)
{
    const long mcu = m0 + b / g.bpm;
    const int w = (int)(b % g.bpm);
    const long my = mcu / g.mcux, mx = mcu % g.mcux;
    if (w < g.hv) { c = 0; return (my * g.vmax + w / g.hmax) * ((long)g.mcux * g.hmax) + mx * g.hmax + w % g.hmax; }
    c = 1 + w - g.hv;
    return (c == 1 ? g.off1 : g.off2) + my * g.mcux + mx;
}

enum { SEG_DONE = 0, SEG_REFILL = -1 };
enum { SEG_WINDOW = 4096, SEG_MARGIN = 528 };
// (a block is at most a 16-bit code + 11 bits, then 63 x (16-bit code + 15 bits): 1980 bits = 248 bytes, 496 with every
//  byte stuffed, and the reader runs at most 8 bytes - 16 stuffed - ahead: a block that starts SEG_MARGIN bytes before the
//  window's end never reaches it)
struct SegState {
    long blk;                                      // next block of the segment
    int pred0, pred1, pred2;
    SegReader br;
};

// Decodes blocks [st.blk, nblk) of one segment into `img` (the image's own block range, ZERO-FILLED by the caller: only
// non-zero positions are written).  lut[c] / lut[3 + c]: DC / AC table of component c; zigzag: kZigzag, where the caller
// keeps it.  -> SEG_DONE, EDITOR_JPEG_CORRUPT (code not found, DC size above 11, index past 63 - decode()'s three), or
// SEG_REFILL when the window ends before the segment does and the next block might cross it (st then names the byte to
// restage from).
__host__ __device__ __forceinline__ int decode_segment_blocks(SegState& st, const ScanGeom& g, const HuffLut* lut, const uint8_t* zigzag, int16_t* img,
                                                              long m0, long nblk)
{
    SegReader& br = st.br;
    while (st.blk < nblk) {
        if (br.lim < br.end && br.p + SEG_MARGIN > br.lim) return SEG_REFILL;
        int c;
        const long dst = scan_block(g, m0, st.blk, c);
        if (dst < 0 || dst >= g.total_blocks) return EDITOR_JPEG_CORRUPT;     // (cannot happen: see scan_block)
        int16_t* blk = img + dst * 64;
        const int sdc = huff_symbol(br, lut[c]);
        if (sdc < 0 || sdc > 11) return EDITOR_JPEG_CORRUPT;
        const int diff = sdc ? seg_extend(br.get(sdc), sdc) : 0;
        int pred = (c == 0 ? st.pred0 : (c == 1 ? st.pred1 : st.pred2)) + diff;
        if (c == 0) st.pred0 = pred; else if (c == 1) st.pred1 = pred; else st.pred2 = pred;
        blk[0] = (int16_t)pred;
        const HuffLut& ac = lut[3 + c];
        for (int kk = 1; kk < 64;) {
            const int rs = huff_symbol(br, ac);
            if (rs < 0) return EDITOR_JPEG_CORRUPT;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) { if (r == 15) { kk += 16; continue; } break; }
            kk += r;
            if (kk > 63) return EDITOR_JPEG_CORRUPT;
            blk[zigzag[kk]] = (int16_t)seg_extend(br.get(sz), sz);      // (kk <= 63 checked above)
            ++kk;
        }
        ++st.blk;
    }
    return SEG_DONE;
}

__host__ __device__ __forceinline__ void seg_begin(SegState& st, long start, long end)
{
    st.blk = 0; st.pred0 = st.pred1 = st.pred2 = 0;
    st.br.p = start; st.br.end = end; st.br.acc = 0; st.br.nbits = 0; st.br.marker = false;
}

// Descriptor tables of a planned batch (host and device entries take the same ones):
//   fdesc (B,16) int32   ncomp, hmax, vmax, mcus_x, mcus_y, restart interval, DC table of component 0..2, AC table of 0..2
//                        (rows of the batch's table pool `huff`, nhuff x 272 bytes)
//   ftab  (3,B)  int64   first coefficient block; where byte 0 of the FILE would sit in `bytes` (only the scan's bytes need
//                        be there, so this may be negative); INCLUSIVE prefix sum of segments (a host-decoded file: none)
//   seg   (S,3)  int64   [byte start, byte end) in the file, first MCU
enum { FT_COEF = 0, FT_BYTE = 1, FT_SEGS = 2, FT_ROWS = 3 };

// Everything the segment decoder trusts, checked on the host copies before anything runs.
bool check_entropy_tables(long nbytes, const int* fdesc, const long* ftab, const long* seg, int nhuff, int B, long nseg, long coef_blocks)
{
    if (nbytes < 0 || B < 1 || nseg < 0 || nhuff < 1 || coef_blocks < 0) return false;
    long done = 0;
    for (int f = 0; f < B; ++f) {
        const long upto = ftab[(long)FT_SEGS * B + f];
        const long ns = upto - done;
        if (ns < 0 || upto > nseg) return false;
        if (ns == 0) continue;
        ScanGeom g;
        const int* fd = fdesc + (long)f * 16;
        if (!make_scan_geom(fd, g)) return false;
        for (int c = 0; c < g.ncomp; ++c)
            if (fd[6 + c] < 0 || fd[6 + c] >= nhuff || fd[9 + c] < 0 || fd[9 + c] >= nhuff) return false;
        const long co = ftab[(long)FT_COEF * B + f], bo = ftab[(long)FT_BYTE * B + f];
        if (co < 0 || co > coef_blocks || g.total_blocks > coef_blocks - co) return false;
        // the segments cover every MCU once: segment k starts at MCU k * Ri
        if (ns != (g.restart ? (g.nmcu + g.restart - 1) / g.restart : 1)) return false;
        for (long k = 0; k < ns; ++k) {
            const long* s = seg + (done + k) * 3;
            if (s[2] != k * g.restart || s[0] > s[1] || bo > nbytes || s[0] < -bo || s[1] > nbytes - bo) return false;
        }
        done = upto;
    }
    return done == nseg;
}

// One restart segment of the batch as either decoder sees it: whose it is, which blocks it holds, where its bytes are.
struct SegDesc {
    int f;                                         // the file
    ScanGeom g;
    long m0, nblk;                                 // first MCU; blocks
    long start, end;                               // its bytes, in `bytes`
    int16_t* img;                                  // the file's first coefficient block
};
// segment s, which belongs to file f (tables validated by check_entropy_tables before anything runs)
__host__ __device__ __forceinline__ bool seg_describe(SegDesc& d, int f, const int* fdesc, const long* ftab, const long* seg, int16_t* coef, int B, long s)
{
    d.f = f;
    if (!make_scan_geom(fdesc + (long)f * 16, d.g)) return false;
    d.m0 = seg[s * 3 + 2];
    const long m1 = d.g.restart && d.m0 + d.g.restart < d.g.nmcu ? d.m0 + d.g.restart : d.g.nmcu;
    d.nblk = (m1 - d.m0) * d.g.bpm;
    const long bo = ftab[(long)FT_BYTE * B + f];
    d.start = bo + seg[s * 3]; d.end = bo + seg[s * 3 + 1];
    d.img = coef + ftab[(long)FT_COEF * B + f] * 64;
    return true;
}

// The kernels' prologue and window staging, `nlanes` lanes of one workgroup.  EVERY lane calls each of these, and none of
// them holds a barrier: the barriers between them stand in the kernels' bodies.
// the zigzag copy and the per-length rows of the scan's six tables (fd: the file's fdesc row) ...
__device__ __forceinline__ void seg_tables_begin(HuffLut* lut, uint8_t* zigzag, const ScanGeom& g, const int* fd, const uint8_t* huff, int lane, int nlanes)
{
    if (nlanes == 64 || lane < 64) zigzag[lane] = kZigzagDev[lane];
    if (lane < 6 && lane % 3 < g.ncomp) lut_lengths(lut[lane], huff + (long)fd[6 + lane] * DHT_BYTES);
}
// ... and, after a barrier, their values and lookahead entries
__device__ __forceinline__ void seg_tables_fill(HuffLut* lut, const ScanGeom& g, const int* fd, const uint8_t* huff, int lane, int nlanes)
{
    for (int t = 0; t < 6; ++t)
        if (t % 3 < g.ncomp) lut_fill(lut[t], huff + (long)fd[6 + t] * DHT_BYTES, lane, nlanes);
}
// zero the segment's blocks, 16 bytes per lane
__device__ __forceinline__ void seg_zero_blocks(const SegDesc& d, int lane, int nlanes)
{
    for (long i = lane; i < d.nblk * 8; i += nlanes) {
        int c;
        const long dst = scan_block(d.g, d.m0, i >> 3, c);
        *reinterpret_cast<uint4*>(d.img + dst * 64 + (i & 7) * 8) = make_uint4(0, 0, 0, 0);
    }
}
// win[0, need) = bytes[wpos, wpos + need), 16 bytes per lane (wpos, win 16-byte aligned), zeros outside [0, nbytes)
__device__ __forceinline__ void seg_stage_window(uint8_t* win, const uint8_t* __restrict__ bytes, long nbytes, long wpos, int need, int lane, int nlanes)
{
    for (int i = lane * 16; i < need; i += nlanes * 16) {
        const long a = wpos + i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a >= 0 && a + 16 <= nbytes) v = *reinterpret_cast<const uint4*>(bytes + a);
        *reinterpret_cast<uint4*>(win + i) = v;
    }
}

// one 64-thread workgroup (one wave) per restart segment of the whole batch
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes, long nbytes, const int* __restrict__ fdesc,
                                                          const long* __restrict__ ftab, const long* __restrict__ seg,
                                                          const uint8_t* __restrict__ huff, int B, long nseg, int16_t* __restrict__ coef,
                                                          int* __restrict__ status)
{
    __shared__ HuffLut lut[6];
    __shared__ __attribute__((aligned(16))) uint8_t win[SEG_WINDOW];
    __shared__ uint8_t zigzag[64];
    __shared__ long next_pos;
    __shared__ int verdict;
    const long s = blockIdx.x;
    if (s >= nseg) return;
    const int lane = threadIdx.x;
    const int f = ragged_find(ftab + (long)FT_SEGS * B, B, s);
    const int* fd = fdesc + (long)f * 16;
    SegDesc d;
    if (!seg_describe(d, f, fdesc, ftab, seg, coef, B, s)) return;        // (validated on the host before the launch)

    seg_tables_begin(lut, zigzag, d.g, fd, huff, lane, EDITOR_WAVE);
    __syncthreads();
    seg_tables_fill(lut, d.g, fd, huff, lane, EDITOR_WAVE);
    seg_zero_blocks(d, lane, EDITOR_WAVE);
    __threadfence_block();
    __syncthreads();

    SegState st;
    seg_begin(st, d.start, d.end);
    long wpos = d.start & ~15L;
    int rc = SEG_REFILL;
    for (long round = 0; round <= d.nblk && rc == SEG_REFILL; ++round) { // (every round decodes at least one block)
        const long need = d.end - wpos < SEG_WINDOW ? d.end - wpos : SEG_WINDOW;   // (the reader stops at the segment's end)
        seg_stage_window(win, bytes, nbytes, wpos, (int)need, lane, EDITOR_WAVE);
        __syncthreads();
        if (lane == 0) {                                                  // one lane walks the bits
            st.br.buf = win; st.br.base = wpos;
            st.br.lim = wpos + SEG_WINDOW < nbytes ? wpos + SEG_WINDOW : nbytes;
            verdict = decode_segment_blocks(st, d.g, lut, zigzag, d.img, d.m0, d.nblk);
            next_pos = st.br.p;
        }
        __syncthreads();
        rc = verdict;
        wpos = next_pos & ~15L;
        __syncthreads();
    }
    if (lane == 0 && rc != SEG_DONE) status[d.f] = EDITOR_JPEG_CORRUPT;
}


// ------------------------------------------------------------------------------------------------------------------
// the same decode, parallel INSIDE a segment: self-synchronising subsequences (Klein & Wiseman; Weissenberger & Schmidt)
// ------------------------------------------------------------------------------------------------------------------
// A segment's bytes [start, end) are cut at start + k * sub_bytes; one lane owns one subsequence: every symbol (a Huffman code
// and its extra bits) that BEGINS in it.  SPLIT_LANES subsequences make a chunk; one workgroup walks its segment chunk by
// chunk and carries the exact state from one chunk into the next, so nothing ever waits for another workgroup.  In a chunk:
//   round 0     lane 0 starts from the carried (exact) state, every other lane guesses (block 0 of an MCU, a DC size next)
//   round r     a lane whose left neighbour's exit state changed starts again from it; lanes 0..r are exact after round r,
//               so the loop is bounded by the subsequence count whatever the data - synchronisation only ends it early
//   then        an exclusive prefix sum of the lanes' completed-block counts names each lane's first block, and one more
//               walk writes the non-zero AC coefficients and the DC DIFFERENCES of the blocks below the segment's count
// A truncated segment's remaining blocks come from the zero tail SegReader::fill feeds; lane 0 decodes them, at most 64 symbols a
// block.  Last, a per-component prefix sum over the segment's blocks in scan order turns the differences into values:
// (int16_t) of a running sum depends on the sum modulo 2^16 only, so it may be regrouped freely.
//   bytes    as above: bounded by the segment's end and by the staged window, zeros past either
//   writes   block index = prefix sum of counts; destination = scan_block(block index) - never from data; below nblk only
//   loops    a walk: every symbol consumes at least one bit, so at most 8 x sub_bytes symbols (the tail: 64 per block);
//            rounds: the subsequence count; chunks: the byte length
enum { SPLIT_LANES = 256, SPLIT_MARGIN = 64, SPLIT_SUB_MIN = 16, SPLIT_SUB_MAX = 128 };
enum { SUB_ERR = 1, SUB_EXH = 2 };
// (a symbol is at most 31 bits and the reader runs at most 56 bits ahead: under 22 bytes with every byte stuffed, plus the
//  15 bytes the window's start is aligned down by - SPLIT_MARGIN bytes staged past a chunk cover every read of its lanes)

inline bool split_sub_ok(int sub) { return sub >= SPLIT_SUB_MIN && sub <= SPLIT_SUB_MAX && (sub & (sub - 1)) == 0; }

// The decoder's state at a point of the stream, in ONE form per point so that equal points compare equal:
//   p      the byte that holds the next bit (after a stuffed FF 00 pair: the byte after the 00)
//   s      bit in that byte (0 = its top bit) | block in the MCU << 3 | coefficient index << 6 (0: a DC size is next) | flags << 12
//          SUB_EXH  the data ended at p (the segment's end, or a marker): only zeros follow, bit is 0
//          SUB_ERR  absorbing: one of decode()'s three errors happened before this point (p and the rest are 0)
struct SubState { long p; int s; };
__host__ __device__ __forceinline__ bool sub_differs(const SubState& a, const SubState& b) { return a.p != b.p || a.s != b.s; }

// what a walk reads: the scan's geometry and tables, and the staged window of the stream (as SegReader's buf / base / lim)
struct SubCtx {
    const ScanGeom* g; const HuffLut* lut; const uint8_t* zigzag;
    const uint8_t* buf; long base, lim, end;
};

// A lane's guess at the state at its boundary `lo`: a block begins there, unless the boundary splits an FF 00 pair.
__host__ __device__ __forceinline__ SubState sub_guess(const SubCtx& cx, long lo)
{
    SubState s = {lo, 0};
    if (lo - 1 >= cx.base && lo < cx.lim && lo < cx.end && cx.buf[lo - 1 - cx.base] == 0xFF && cx.buf[lo - cx.base] == 0x00) s.p = lo + 1;
    return s;
}

// Walks the symbols that begin before byte `hi`, from state s; s becomes the state at the first symbol that does not, and
// the number of blocks COMPLETED on the way comes back.  At most `budget` symbols.  tail: no `hi` - the walk goes on through
// the zeros past the data (and starts only from a state that is there).  WRITE: `blk` is the block s is in; coefficients of
// blocks below nblk are written into `img` (zero-filled; the DC position gets the DIFFERENCE) and the walk ends at nblk;
// `bad` is set when one of decode()'s three errors is met in such a block.  Without WRITE an error just ends in SUB_ERR: a
// lane that guessed wrong has not found corruption.
template <bool WRITE>
__host__ __device__ __forceinline__ long sub_walk(SubState& s, const SubCtx& cx, long hi, bool tail, bool exact, long budget, int16_t* img, long m0,
                                                 long blk, long nblk, bool& bad)
{
    bad = false;
    const int flags = s.s >> 12;
    if ((flags & SUB_ERR) || ((flags & SUB_EXH) && !tail)) return 0;
    const ScanGeom& g = *cx.g;
    SubReader br;
    br.buf = cx.buf; br.base = cx.base; br.lim = cx.lim; br.end = cx.end;
    br.seek(s.p, s.s & 7);
    int w = (s.s >> 3) & 7, k = (s.s >> 6) & 63;
    long done = 0;
    int16_t* out = nullptr;
    bool fresh = true;
    for (long it = 0; it < budget; ++it) {
        if (WRITE && blk >= nblk) break;
        if (br.nbits <= 24) br.fill();
        if (!tail) {
            if (br.exhausted()) break;
            if (br.p >= hi) {                                             // (the cursor is never past br.p)
                long cp; int cb;
                br.cursor(cp, cb);
                if (cp >= hi) break;
            }
        }
        const int c = w < g.hv ? 0 : 1 + w - g.hv;
        if (WRITE && fresh) {
            int cc;
            const long dst = scan_block(g, m0, blk, cc);
            if (dst < 0 || dst >= g.total_blocks) { bad = true; s.p = 0; s.s = SUB_ERR << 12; return done; }   // (cannot happen: see scan_block)
            out = img + dst * 64;
            fresh = false;
        }
        if (k == 0) {
            const int sdc = huff_symbol(br, cx.lut[c]);
            if (sdc < 0 || sdc > 11) { bad = true; if (exact) { s.p = 0; s.s = SUB_ERR << 12; return done; } k = 0; w = 0; continue; }
            const int diff = sdc ? seg_extend(br.get(sdc), sdc) : 0;
            if (WRITE) out[0] = (int16_t)diff;
            k = 1;
        } else {
            const int rs = huff_symbol(br, cx.lut[3 + c]);
            if (rs < 0) { bad = true; if (exact) { s.p = 0; s.s = SUB_ERR << 12; return done; } k = 0; w = 0; continue; }
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                k = r == 15 ? k + 16 : 64;
            } else {
                k += r;
                if (k > 63) { bad = true; if (exact) { s.p = 0; s.s = SUB_ERR << 12; return done; } k = 0; w = 0; continue; }
                const int v = seg_extend(br.get(sz), sz);
                if (WRITE) out[cx.zigzag[k]] = (int16_t)v;                 // (k <= 63 checked above)
                ++k;
            }
        }
        if (k >= 64) { k = 0; w = w + 1 == g.bpm ? 0 : w + 1; ++done; ++blk; fresh = true; }
    }
    long cp; int cb;
    br.cursor(cp, cb);
    s.p = cp; s.s = cb | (w << 3) | (k << 6) | (br.exhausted() ? SUB_EXH << 12 : 0);
    return done;
}

// the DC differences of blocks [b0, b1) of a segment (scan order), summed per component modulo 2^32 ...
__host__ __device__ __forceinline__ void dc_lane_sum(const ScanGeom& g, const int16_t* img, long m0, long b0, long b1, uint32_t* sum)
{
    for (long b = b0; b < b1; ++b) {
        int c;
        const long dst = scan_block(g, m0, b, c);
        sum[c] += (uint32_t)(int)img[dst * 64];
    }
}
// ... and replaced by the values, pred[c] being the sum over the segment's blocks before b0
__host__ __device__ __forceinline__ void dc_lane_apply(const ScanGeom& g, int16_t* img, long m0, long b0, long b1, uint32_t* pred)
{
    for (long b = b0; b < b1; ++b) {
        int c;
        const long dst = scan_block(g, m0, b, c);
        pred[c] += (uint32_t)(int)img[dst * 64];
        img[dst * 64] = (int16_t)(uint16_t)pred[c];
    }
}

// exclusive prefix sum of one value per lane over the workgroup (tmp: 2 x SPLIT_LANES); every lane calls it
__device__ __forceinline__ uint32_t split_scan(uint32_t v, uint32_t* tmp, int lane)
{
    int cur = 0;
    tmp[lane] = v;
    __syncthreads();
    for (int d = 1; d < SPLIT_LANES; d <<= 1) {
        uint32_t x = tmp[cur * SPLIT_LANES + lane];
        if (lane >= d) x += tmp[cur * SPLIT_LANES + lane - d];
        cur ^= 1;
        tmp[cur * SPLIT_LANES + lane] = x;
        __syncthreads();
    }
    const uint32_t incl = tmp[cur * SPLIT_LANES + lane];
    __syncthreads();
    return incl - v;
}

// dynamic LDS of jpeg_entropy_split_kernel: the window, then (every offset a multiple of 16) the tables and the lanes' states
__host__ __device__ inline long split_window_bytes(int sub_bytes) { return (long)SPLIT_LANES * sub_bytes + SPLIT_MARGIN; }
enum { SPLIT_LDS_FIXED = 6 * (int)sizeof(HuffLut) + SPLIT_LANES * 8 + SPLIT_LANES * 4 + 2 * SPLIT_LANES * 4 + 64 + 32 };
static_assert(sizeof(HuffLut) % 16 == 0, "the carve below keeps 16-byte offsets");

// one SPLIT_LANES-thread workgroup per restart segment of the whole batch; stats (nseg,2): rounds run, chunks walked
__global__ __launch_bounds__(SPLIT_LANES) void jpeg_entropy_split_kernel(const uint8_t* __restrict__ bytes, long nbytes, const int* __restrict__ fdesc,
                                                                         const long* __restrict__ ftab, const long* __restrict__ seg,
                                                                         const uint8_t* __restrict__ huff, int B, long nseg, int sub_bytes,
                                                                         int16_t* __restrict__ coef, int* __restrict__ status, long* __restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t split_lds[];
    const long wbytes = split_window_bytes(sub_bytes);
    uint8_t* win = split_lds;
    HuffLut* lut = reinterpret_cast<HuffLut*>(split_lds + wbytes);
    long* sh_p = reinterpret_cast<long*>(lut + 6);
    int* sh_s = reinterpret_cast<int*>(sh_p + SPLIT_LANES);
    uint32_t* sh_scan = reinterpret_cast<uint32_t*>(sh_s + SPLIT_LANES);
    uint8_t* zigzag = reinterpret_cast<uint8_t*>(sh_scan + 2 * SPLIT_LANES);
    long* sh_car = reinterpret_cast<long*>(zigzag + 64);                  // carried: p, s, blocks done
    const long s = blockIdx.x;
    if (s >= nseg) return;
    const int lane = threadIdx.x;
    const int f = ragged_find(ftab + (long)FT_SEGS * B, B, s);
    const int* fd = fdesc + (long)f * 16;
    SegDesc d;
    if (!seg_describe(d, f, fdesc, ftab, seg, coef, B, s)) return;        // (validated on the host before the launch)
    const ScanGeom& g = d.g;
    const long m0 = d.m0, nblk = d.nblk, start = d.start, end = d.end;
    int16_t* img = d.img;

    seg_tables_begin(lut, zigzag, g, fd, huff, lane, SPLIT_LANES);
    __syncthreads();
    seg_tables_fill(lut, g, fd, huff, lane, SPLIT_LANES);
    seg_zero_blocks(d, lane, SPLIT_LANES);
    __threadfence_block();
    __syncthreads();

    SubCtx cx;
    cx.g = &g; cx.lut = lut; cx.zigzag = zigzag; cx.buf = win; cx.end = end;
    const long chunk_bytes = (long)SPLIT_LANES * sub_bytes;
    const long nchunks = (end - start + chunk_bytes - 1) / chunk_bytes;
    const long budget = 8L * sub_bytes + 8;
    SubState car = {start, 0};                                            // (uniform: every lane holds the same copy)
    long base_blk = 0, rounds = 0, chunks = 0;
    for (long ch = 0; ch < nchunks; ++ch) {
        if ((car.s >> 12) || base_blk >= nblk) break;                     // an error, the data's end or the last block: nothing left to find
        const long c0 = start + ch * chunk_bytes;
        const long c1 = c0 + chunk_bytes < end ? c0 + chunk_bytes : end;
        const long wpos = c0 & ~15L;
        const long need = c1 - wpos + SPLIT_MARGIN - 16 < wbytes ? c1 - wpos + SPLIT_MARGIN - 16 : wbytes;
        seg_stage_window(win, bytes, nbytes, wpos, (int)need, lane, SPLIT_LANES);
        __syncthreads();
        cx.base = wpos;
        cx.lim = wpos + ((need + 15) & ~15L) < nbytes ? wpos + ((need + 15) & ~15L) : nbytes;
        const long nsub = (c1 - c0 + sub_bytes - 1) / sub_bytes;
        const bool active = lane < nsub;
        const long lo = c0 + (long)lane * sub_bytes;
        const long hi = lo + sub_bytes < end ? lo + sub_bytes : end;
        // `hit`: this lane's last walk was a guess that met an error and went on (block 0, a DC size next): its exit state is
        // not what an exact walk from the same entry gives, so the rounds go on until the exact front (lane r in round r) redoes it
        bool bad = false, hit = false;
        SubState entry = car, exit;
        if (lane > 0) entry = sub_guess(cx, lo);
        exit = entry;
        long cnt = 0;
        if (active) { cnt = sub_walk<false>(exit, cx, hi, false, lane == 0, budget, img, m0, 0, nblk, bad); hit = bad && lane > 0; }
        sh_p[lane] = exit.p; sh_s[lane] = exit.s;
        __syncthreads();
        ++rounds;
        for (long r = 1; r < nsub; ++r) {
            SubState ne = entry;
            if (active && lane > 0) { ne.p = sh_p[lane - 1]; ne.s = sh_s[lane - 1]; }
            const bool changed = sub_differs(ne, entry) || (hit && lane <= r);
            if (!__syncthreads_or(changed || hit)) break;                 // (every neighbour is read before any is rewritten)
            if (changed) {
                entry = exit = ne;
                cnt = sub_walk<false>(exit, cx, hi, false, lane <= r, budget, img, m0, 0, nblk, bad);
                hit = bad && lane > r;
                sh_p[lane] = exit.p; sh_s[lane] = exit.s;
            }
            __syncthreads();
            ++rounds;
        }
        const long first = base_blk + split_scan(active ? (uint32_t)cnt : 0u, sh_scan, lane);
        if (active) {
            SubState t = entry;
            sub_walk<true>(t, cx, hi, false, true, budget, img, m0, first, nblk, bad);
            if (bad) status[f] = EDITOR_JPEG_CORRUPT;
        }
        if (lane == nsub - 1) { sh_car[0] = exit.p; sh_car[1] = exit.s; sh_car[2] = first + cnt; }
        __syncthreads();
        car.p = sh_car[0]; car.s = (int)sh_car[1]; base_blk = sh_car[2];
        ++chunks;
        __syncthreads();
    }
    // a segment that ends early: its remaining blocks from the zeros past the data
    if (lane == 0 && !((car.s >> 12) & SUB_ERR) && base_blk < nblk) {
        SubCtx tc = cx;
        tc.base = 0; tc.lim = 0;                                          // (no byte is read)
        SubState t = {car.p, car.s & ~7};
        bool bad = false;
        sub_walk<true>(t, tc, 0, true, true, (nblk - base_blk) * 64 + 64, img, m0, base_blk, nblk, bad);
        if (bad) status[f] = EDITOR_JPEG_CORRUPT;
    }
    __threadfence_block();
    __syncthreads();
    // DC differences -> values
    const long per = (nblk + SPLIT_LANES - 1) / SPLIT_LANES;
    const long b0 = lane * per < nblk ? lane * per : nblk;
    const long b1 = b0 + per < nblk ? b0 + per : nblk;
    uint32_t sum[3] = {0, 0, 0}, pred[3] = {0, 0, 0};
    dc_lane_sum(g, img, m0, b0, b1, sum);
    for (int c = 0; c < g.ncomp; ++c) pred[c] = split_scan(sum[c], sh_scan, lane);
    dc_lane_apply(g, img, m0, b0, b1, pred);
    if (lane == 0) { stats[s * 2] = rounds; stats[s * 2 + 1] = chunks; }
}

// The host twins' walk over a planned batch (tables checked by the caller): every file's status cleared; for a file with
// segments its six tables built and its blocks zeroed, then body(s, segment, tables) for each of its segments in order.
template <class Body>
void for_each_segment(const int* fdesc, const long* ftab, const long* seg, const uint8_t* huff, int B, int16_t* coef, int* status, Body body)
{
    HuffLut lut[6];
    long done = 0;
    for (int f = 0; f < B; ++f) {
        status[f] = 0;
        const long upto = ftab[(long)FT_SEGS * B + f];
        const int* fd = fdesc + (long)f * 16;
        for (long s = done; s < upto; ++s) {
            SegDesc d;
            seg_describe(d, f, fdesc, ftab, seg, coef, B, s);
            if (s == done) {
                for (int t = 0; t < 6; ++t)
                    if (t % 3 < d.g.ncomp) {
                        const uint8_t* dht = huff + (long)fd[6 + t] * DHT_BYTES;
                        lut_lengths(lut[t], dht);
                        lut_fill(lut[t], dht, 0, 1);
                    }
                memset(d.img, 0, (size_t)d.g.total_blocks * 128);
            }
            body(s, d, lut);
        }
        done = upto;
    }
}

// What the two device entries check before they launch, and the cleared status vector; 0 or the error to return.
int entropy_device_begin(const uint8_t* bytes, long nbytes, const int* fdesc_host, const long* ftab_host, const long* seg_host, const int* fdesc,
                         const long* ftab, const long* seg, const uint8_t* huff, int nhuff, int B, long nseg, int16_t* coef, long coef_blocks,
                         int* status, hipStream_t stream)
{
    if (!bytes || !fdesc_host || !ftab_host || !seg_host || !fdesc || !ftab || !seg || !huff || !coef || !status)
        return (int)hipErrorInvalidValue;
    // the kernels stage 16 bytes per lane: the byte buffer is 16-byte aligned and a whole number of such pieces
    if (((uintptr_t)bytes & 15) || (nbytes & 15) || ((uintptr_t)coef & 15)) return (int)hipErrorInvalidValue;
    if (!check_entropy_tables(nbytes, fdesc_host, ftab_host, seg_host, nhuff, B, nseg, coef_blocks)) return (int)hipErrorInvalidValue;
    if (nseg > 0x7fffffffL) return (int)hipErrorInvalidValue;
    return (int)hipMemsetAsync(status, 0, (size_t)B * sizeof(int), stream);
}

// the three quantisation tables as the reconstruct kernels take them (a component the file lacks: ones)
void fill_qt(const Jpeg& j, uint16_t* qt)
{
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) qt[c * 64 + i] = c < j.ncomp ? j.qt[j.comp[c].tq][i] : 1;
}

}  // namespace

extern "C" int editor_jpeg_parse(const uint8_t* data, long n, int* info)
{
    if (!data || !info) return EDITOR_JPEG_CORRUPT;
    Jpeg j;
    const int rc = decode(data, n, j, nullptr, 0);
    if (rc) return rc;
    fill_info(j, info);
    return 0;
}

extern "C" int editor_jpeg_entropy_decode(const uint8_t* data, long n, int16_t* coef, long coef_blocks, uint16_t* qt, int* info)
{
    if (!data || !coef || !qt || !info) return EDITOR_JPEG_CORRUPT;
    Jpeg j;
    int rc = decode(data, n, j, nullptr, 0);                  // geometry first: the caller's buffer must hold it
    if (rc) return rc;
    if (j.total_blocks > coef_blocks) return EDITOR_JPEG_CORRUPT;
    // blocks no scan covers (the MCU padding of a per-component scan) are zero, never what the caller's buffer held
    memset(coef, 0, (size_t)j.total_blocks * 128);
    Jpeg k;
    rc = decode(data, n, k, coef, coef_blocks);
    if (rc) return rc;
    fill_info(k, info);
    fill_qt(k, qt);
    return 0;
}

extern "C" int editor_jpeg_planes_bytes(const int* info, long* bytes)
{
    JpegGeom g;
    if (!info || !bytes || !make_geom(info, g)) return EDITOR_JPEG_CORRUPT;
    *bytes = g.plane_bytes;
    return 0;
}

extern "C" int editor_jpeg_reconstruct(const int16_t* coef, const uint16_t* qt, const int* info /* host */, int B, uint8_t* planes,
                                       int crop_w, uint8_t* out, hipStream_t stream)
{
    JpegGeom g;
    if (!coef || !qt || !info || !planes || !out || B < 1 || !make_geom(info, g)) return (int)hipErrorInvalidValue;
    if (crop_w <= 0) crop_w = g.W;
    const int ncrop = g.W / crop_w;
    if (ncrop < 1) return (int)hipErrorInvalidValue;
    const long nb = (long)B * g.blocks_per_image;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nb + 127) / 128)), dim3(128), 0, stream, coef, qt, g, B, planes);
    EDITOR_LAUNCH_CHECK();
    const long npx = (long)B * g.H * crop_w * ncrop;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, planes, g, B, crop_w, ncrop, out);
    EDITOR_LAUNCH_CHECK();
    return 0;
}

extern "C" int editor_jpeg_reconstruct_ragged(const int16_t* coef, const uint16_t* qt, const int* info_host, const long* tab_host,
                                              const int* info, const long* tab, int B, uint8_t* planes, uint8_t* out, hipStream_t stream)
{
    if (!coef || !qt || !info_host || !tab_host || !info || !tab || !planes || !out || B < 1) return (int)hipErrorInvalidValue;
    // the kernels trust the tables: every row a geometry make_geom accepts, the prefix sums those geometries' own counts,
    // offsets non-negative, plane bases 8-byte aligned
    long blocks = 0, pixels = 0;
    for (int i = 0; i < B; ++i) {
        JpegGeom g;
        if (!make_geom(info_host + (long)i * 16, g)) return (int)hipErrorInvalidValue;
        if (g.hmax < 1 || g.hmax > 2 || g.vmax < 1 || g.vmax > 2 || (long)g.mcux * 8 * g.hmax < g.W || (long)g.mcuy * 8 * g.vmax < g.H)
            return (int)hipErrorInvalidValue;                         // (the planes must cover the pixels the colour pass reads)
        blocks += g.blocks_per_image; pixels += (long)g.W * g.H;
        const long po = tab_host[(long)RT_PLANE * B + i];
        if (tab_host[(long)RT_COEF * B + i] < 0 || po < 0 || (po & 7) || tab_host[(long)RT_OUT * B + i] < 0 ||
            tab_host[(long)RT_BLOCKS * B + i] != blocks || tab_host[(long)RT_PIXELS * B + i] != pixels)
            return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(jpeg_idct_ragged_kernel, dim3((unsigned)((blocks + 127) / 128)), dim3(128), 0, stream, coef, qt, info, tab, B, blocks, planes);
    EDITOR_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_color_ragged_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, planes, info, tab, B, pixels, out);
    EDITOR_LAUNCH_CHECK();
    return 0;
}

// ---- device-side entropy decode of sequential scans ----------------------------------------------------------------
extern "C" int editor_jpeg_plan(const uint8_t* data, long n, int* info, int* plan, uint16_t* qt, uint8_t* huff, long* seg, long seg_cap)
{
    if (!data || !info || !plan || !qt || !huff || (!seg && seg_cap > 0)) return EDITOR_JPEG_CORRUPT;
    Jpeg j;
    ScanPlan sp;
    j.plan = &sp;
    const int rc = decode(data, n, j, nullptr, 0);
    if (rc) return rc;
    fill_info(j, info);
    fill_qt(j, qt);
    memcpy(huff, sp.dht, sizeof(sp.dht));
    // one pass over the first scan's entropy-coded bytes; a byte after 0xFF is classified as BitReader::fill does: 00 is a
    // stuffed data byte, anything else (or nothing) ends the data - an RSTn ends a segment, the rest end the scan
    const long nmcu = (long)j.mcux * j.mcuy;
    long p = sp.ecs, seg_start = sp.ecs, nseg = 0, markers = 0, end = n;
    bool cyclic = true;
    while (p < n) {
        const uint8_t* ff = (const uint8_t*)memchr(data + p, 0xFF, (size_t)(n - p));
        if (!ff) break;
        p = ff - data;
        if (p + 1 < n && data[p + 1] == 0x00) { p += 2; continue; }
        if (p + 1 < n && data[p + 1] >= 0xD0 && data[p + 1] <= 0xD7) {
            if (nseg < seg_cap) { seg[nseg * 3] = seg_start; seg[nseg * 3 + 1] = p; seg[nseg * 3 + 2] = nseg * sp.restart; }
            if (data[p + 1] != 0xD0 + (markers & 7)) cyclic = false;
            ++nseg; ++markers;
            p += 2; seg_start = p;
            continue;
        }
        end = p;
        break;
    }
    if (nseg < seg_cap) { seg[nseg * 3] = seg_start; seg[nseg * 3 + 1] = end; seg[nseg * 3 + 2] = nseg * sp.restart; }
    ++nseg;
    const long expect = sp.restart ? (nmcu + sp.restart - 1) / sp.restart - 1 : 0;
    const bool eligible = !j.progressive && sp.nsos == 1 && sp.whole_frame_in_order && sp.tables_present && markers == expect && cyclic;
    memset(plan, 0, 16 * sizeof(int));
    plan[0] = eligible; plan[1] = (int)(nseg > 0x7fffffff ? 0x7fffffff : nseg); plan[2] = sp.restart; plan[3] = (int)nmcu;
    for (int c = 0; c < 3; ++c) { plan[4 + c] = sp.td[c]; plan[7 + c] = sp.ta[c]; }
    plan[10] = sp.nsos;
    return 0;
}

extern "C" int editor_jpeg_entropy_segments(const uint8_t* bytes, long nbytes, const int* fdesc, const long* ftab, const long* seg,
                                            const uint8_t* huff, int nhuff, int B, long nseg, int16_t* coef, long coef_blocks, int* status)
{
    if (!bytes || !fdesc || !ftab || !seg || !huff || !coef || !status) return (int)hipErrorInvalidValue;
    if (!check_entropy_tables(nbytes, fdesc, ftab, seg, nhuff, B, nseg, coef_blocks)) return (int)hipErrorInvalidValue;
    for_each_segment(fdesc, ftab, seg, huff, B, coef, status, [&](long, const SegDesc& d, const HuffLut* lut) {
        SegState st;
        seg_begin(st, d.start, d.end);
        st.br.buf = bytes; st.br.base = 0; st.br.lim = nbytes;
        if (decode_segment_blocks(st, d.g, lut, kZigzag, d.img, d.m0, d.nblk) != SEG_DONE) status[d.f] = EDITOR_JPEG_CORRUPT;
    });
    return 0;
}

extern "C" int editor_jpeg_entropy_device(const uint8_t* bytes, long nbytes, const int* fdesc_host, const long* ftab_host, const long* seg_host,
                                          const int* fdesc, const long* ftab, const long* seg, const uint8_t* huff, int nhuff, int B,
                                          long nseg, int16_t* coef, long coef_blocks, int* status, hipStream_t stream)
{
    const int rc = entropy_device_begin(bytes, nbytes, fdesc_host, ftab_host, seg_host, fdesc, ftab, seg, huff, nhuff, B, nseg, coef, coef_blocks,
                                        status, stream);
    if (rc) return rc;
    if (nseg == 0) return 0;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)nseg), dim3(EDITOR_WAVE), 0, stream, bytes, nbytes, fdesc, ftab, seg, huff, B, nseg,
                       coef, status);
    EDITOR_LAUNCH_CHECK();
    return 0;
}

// ---- the same, parallel inside a segment (entropy="device_split") -------------------------------------------------------------
// workspace: (nseg,2) int64 statistics - rounds run and chunks walked per segment, written by either entry - then the host
// twin's table of lanes (entry p, exit p: int64; entry s, exit s, blocks completed, guess met an error: int32)
extern "C" int editor_jpeg_entropy_split_workspace(long nseg, int sub_bytes, long* bytes)
{
    if (!bytes || nseg < 0 || nseg > 0x7fffffffL || !split_sub_ok(sub_bytes)) return (int)hipErrorInvalidValue;
    *bytes = nseg * 16 + (long)SPLIT_LANES * 32;
    return 0;
}

extern "C" int editor_jpeg_entropy_split_segments(const uint8_t* bytes, long nbytes, const int* fdesc, const long* ftab, const long* seg,
                                                  const uint8_t* huff, int nhuff, int B, long nseg, int sub_bytes, void* workspace,
                                                  long workspace_bytes, int16_t* coef, long coef_blocks, int* status)
{
    if (!bytes || !fdesc || !ftab || !seg || !huff || !workspace || !coef || !status) return (int)hipErrorInvalidValue;
    long ws = 0;
    if (editor_jpeg_entropy_split_workspace(nseg, sub_bytes, &ws) || workspace_bytes < ws || ((uintptr_t)workspace & 7)) return (int)hipErrorInvalidValue;
    if (!check_entropy_tables(nbytes, fdesc, ftab, seg, nhuff, B, nseg, coef_blocks)) return (int)hipErrorInvalidValue;
    long* stats = (long*)workspace;
    long* en_p = stats + nseg * 2;
    long* ex_p = en_p + SPLIT_LANES;
    int* en_s = (int*)(ex_p + SPLIT_LANES);
    int* ex_s = en_s + SPLIT_LANES;
    int* cnt = ex_s + SPLIT_LANES;
    int* hit = cnt + SPLIT_LANES;                                       // (see the kernel)
    const long chunk_bytes = (long)SPLIT_LANES * sub_bytes, budget = 8L * sub_bytes + 8;
    for_each_segment(fdesc, ftab, seg, huff, B, coef, status, [&](long s, const SegDesc& d, const HuffLut* lut) {
        const ScanGeom& g = d.g;
        const int f = d.f;
        const long m0 = d.m0, nblk = d.nblk, start = d.start, end = d.end;
        int16_t* img = d.img;
        SubCtx cx;
        cx.g = &g; cx.lut = lut; cx.zigzag = kZigzag; cx.buf = bytes; cx.base = 0; cx.lim = nbytes; cx.end = end;
        const long nchunks = (end - start + chunk_bytes - 1) / chunk_bytes;
        SubState car = {start, 0};
        long base_blk = 0, rounds = 0, chunks = 0;
        bool bad = false;
        // the kernel's chunk loop, its lanes one after another
        for (long ch = 0; ch < nchunks; ++ch) {
            if ((car.s >> 12) || base_blk >= nblk) break;
            const long c0 = start + ch * chunk_bytes;
            const long c1 = c0 + chunk_bytes < end ? c0 + chunk_bytes : end;
            const long nsub = (c1 - c0 + sub_bytes - 1) / sub_bytes;
            auto hi_of = [&](long lane) { const long lo = c0 + lane * sub_bytes; return lo + sub_bytes < end ? lo + sub_bytes : end; };
            for (long lane = 0; lane < nsub; ++lane) {
                SubState e = lane ? sub_guess(cx, c0 + lane * sub_bytes) : car, x = e;
                cnt[lane] = (int)sub_walk<false>(x, cx, hi_of(lane), false, lane == 0, budget, img, m0, 0, nblk, bad);
                hit[lane] = bad && lane > 0;
                en_p[lane] = e.p; en_s[lane] = e.s; ex_p[lane] = x.p; ex_s[lane] = x.s;
            }
            ++rounds;
            for (long r = 1; r < nsub; ++r) {
                bool any = false;
                for (long lane = nsub - 1; lane > 0; --lane) {         // (downwards: lane - 1 still holds the last round's exit)
                    const SubState ne = {ex_p[lane - 1], ex_s[lane - 1]}, e = {en_p[lane], en_s[lane]};
                    any = any || hit[lane];
                    if (!sub_differs(ne, e) && !(hit[lane] && lane <= r)) continue;
                    any = true;
                    SubState x = ne;
                    cnt[lane] = (int)sub_walk<false>(x, cx, hi_of(lane), false, lane <= r, budget, img, m0, 0, nblk, bad);
                    hit[lane] = bad && lane > r;
                    en_p[lane] = ne.p; en_s[lane] = ne.s; ex_p[lane] = x.p; ex_s[lane] = x.s;
                }
                if (!any) break;
                ++rounds;
            }
            long first = base_blk;
            for (long lane = 0; lane < nsub; ++lane) {
                SubState t = {en_p[lane], en_s[lane]};
                bool lane_bad = false;
                sub_walk<true>(t, cx, hi_of(lane), false, true, budget, img, m0, first, nblk, lane_bad);
                if (lane_bad) status[f] = EDITOR_JPEG_CORRUPT;
                first += cnt[lane];
            }
            car.p = ex_p[nsub - 1]; car.s = ex_s[nsub - 1]; base_blk = first;
            ++chunks;
        }
        if (!((car.s >> 12) & SUB_ERR) && base_blk < nblk) {
            SubCtx tc = cx;
            tc.base = 0; tc.lim = 0;
            SubState t = {car.p, car.s & ~7};
            bool tail_bad = false;
            sub_walk<true>(t, tc, 0, true, true, (nblk - base_blk) * 64 + 64, img, m0, base_blk, nblk, tail_bad);
            if (tail_bad) status[f] = EDITOR_JPEG_CORRUPT;
        }
        const long per = (nblk + SPLIT_LANES - 1) / SPLIT_LANES;
        uint32_t pred[3] = {0, 0, 0};
        uint32_t sums[SPLIT_LANES][3];
        for (long lane = 0; lane < SPLIT_LANES; ++lane) {
            const long b0 = lane * per < nblk ? lane * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
            sums[lane][0] = sums[lane][1] = sums[lane][2] = 0;
            dc_lane_sum(g, img, m0, b0, b1, sums[lane]);
        }
        for (long lane = 0; lane < SPLIT_LANES; ++lane) {
            const long b0 = lane * per < nblk ? lane * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
            uint32_t mine[3] = {pred[0], pred[1], pred[2]};           // the exclusive prefix sum of the lanes' sums
            dc_lane_apply(g, img, m0, b0, b1, mine);
            for (int c = 0; c < 3; ++c) pred[c] += sums[lane][c];
        }
        stats[s * 2] = rounds; stats[s * 2 + 1] = chunks;
    });
    return 0;
}

extern "C" int editor_jpeg_entropy_split_device(const uint8_t* bytes, long nbytes, const int* fdesc_host, const long* ftab_host,
                                                const long* seg_host, const int* fdesc, const long* ftab, const long* seg, const uint8_t* huff,
                                                int nhuff, int B, long nseg, int sub_bytes, void* workspace, long workspace_bytes, int16_t* coef,
                                                long coef_blocks, int* status, hipStream_t stream)
{
    long ws = 0;
    if (!workspace || editor_jpeg_entropy_split_workspace(nseg, sub_bytes, &ws) || workspace_bytes < ws || ((uintptr_t)workspace & 7)) return (int)hipErrorInvalidValue;
    const int rc = entropy_device_begin(bytes, nbytes, fdesc_host, ftab_host, seg_host, fdesc, ftab, seg, huff, nhuff, B, nseg, coef, coef_blocks,
                                        status, stream);
    if (rc) return rc;
    if (nseg == 0) return 0;
    const size_t lds = (size_t)split_window_bytes(sub_bytes) + SPLIT_LDS_FIXED;
    hipLaunchKernelGGL(jpeg_entropy_split_kernel, dim3((unsigned)nseg), dim3(SPLIT_LANES), lds, stream, bytes, nbytes, fdesc, ftab, seg, huff, B,
                       nseg, sub_bytes, coef, status, (long*)workspace);
    EDITOR_LAUNCH_CHECK();
    return 0;
}
