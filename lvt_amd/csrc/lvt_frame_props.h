// lvt_frame_props.h -- the properties a handle, or one sequence of a batch, has besides its parameters (included by lvt_host.hip): rectifiers for raw frames,
// a pixel format for colour frames, a reduction for large frames, a depth camera for unregistered depth, an equalisation record for dim frames, a depth guard and feature masks behind the
// gather step, label masks whose images travel with each frame, the pose-uncertainty record.
//
// THE CONTRACT they share ("Frame properties"): a call is checked before anything changes and refused with a reason (-1, the handle as it
// was, lvt_amd_last_error says why); it needs a quiet handle (no frame in flight); an lvt_create handle is decided under its record's lock; a property is
// configuration, not state (reset and snapshots leave it alone); and a context without the property launches what it always did.
// Here: the one path every such call takes (frames_in_flight, with_auto_handle, set_property), the one packer of the by-value descriptor tables and the one frame of the two filters behind the gather, the
// setters and getters, and the launches the properties add to the head of a frame's feature stage (enqueue_frame calls them in this file's order).
#pragma once

namespace lvt {

// ---- one path for "change a property of a quiet handle" ---------------------------------------------------------------------------------------------
static int refuse_unchanged(lvt_handle h, const char *who, const std::string &why) { return refuse(h, who, why + " (nothing was changed)"); }
// a synchronous call's frame whose pose has been returned is nobody's to collect: it is drained; any other un-collected or held frame is in flight
static bool frames_in_flight(Context *c) {
    if (c->early_pending) drain(c);
    return c->done < c->enq || c->pend.valid;
}
// fn(handle) on the tracker behind h.  An lvt_create handle: decided under its record's lock -- a handle that has not been used yet may be given a seat by
// another thread's lvt_create at any time --, and a successful call is a use: the handle keeps its own chain (a refusal is no use)
template <typename Fn>
static int with_auto_handle(lvt_handle h, Fn fn) {
    if (!is_auto(h)) return fn(h);
    AutoHandle *A = static_cast<AutoHandle *>(h);
    std::lock_guard<std::mutex> g(A->mu);
    const int rc = fn(A->impl);
    if (rc == 0) A->started = true;
    return rc;
}
// what distinguishes one property call from another before its own checks begin
struct PropertyCall {
    const char *who;
    int sensor;                 // the sensor the property belongs to (0: either)
    Refusals why;               // to a pooled handle / a handle of the other sensor / a batch handle in the solo spelling
    const char *batch_on_solo;  // to the batch spelling on a solo handle; nullptr: accepted (for seq == 0, by the range check)
};
// The preamble: the handle's kind, the spelling, the sequence -- in this order, then body(h, c), which makes the call's own validity checks, then asks
// frames_in_flight, then changes the context.  The order of objections is behaviour: callers see the first one.
template <typename Body>
static int set_property(lvt_handle h, const PropertyCall &k, int seq, bool batch_call, Body body) {
    return with_auto_handle(h, [&](lvt_handle t) -> int {
        Context *c = frame_context(t, k.who, k.sensor, batch_call, k.why);
        if (!c) return -1;
        DeviceGuard guard(c);
        try {
            if (batch_call && k.batch_on_solo && c->B == 1 && !c->mixed) return refuse_unchanged(t, k.who, k.batch_on_solo);
            if (seq < 0 || seq >= c->B) return refuse_unchanged(t, k.who, "no sequence " + std::to_string(seq) + " in this handle");
            return body(t, c);
        } catch (...) {
        }
        return -1;
    });
}
// sequence seq's planes (each of its own plane_pitch x H elements + pad) in a [B][copies][stride] vector: sized at its first use, `eyes` <= stride planes per
// parity allocated where they do not exist yet (copies == 1: planes no frame in flight writes, one per eye)
template <typename T>
static void give_planes(Context *c, std::vector<T *> &planes, int stride, int seq, int eyes, size_t pad, int copies = NPAR) {
    if (planes.empty()) planes.assign((size_t)c->B * copies * stride, nullptr);
    const size_t plane = (size_t)c->h_seqs[seq].plane_pitch * c->seq_prm(seq).H;
    for (int par = 0; par < copies; par++)
        for (int e = 0; e < eyes; e++) {
            T *&d = planes[((size_t)seq * copies + par) * stride + e];
            if (!d) d = c->dalloc<T>(plane + pad);
        }
}
// the per-sequence values live in vectors that are empty until the first set; the count of sequences that have the property is what the frame path tests
template <typename T, typename Has>
static int put_seq_value(Context *c, std::vector<T> &v, int per_seq, const T &none, int seq, std::initializer_list<T> vals, Has has) {
    if (v.empty()) v.assign((size_t)c->B * per_seq, none);
    std::copy(vals.begin(), vals.end(), v.begin() + (size_t)seq * per_seq);
    int n = 0;
    for (int s = 0; s < c->B; s++) n += has(v[(size_t)s * per_seq]) ? 1 : 0;
    return n;
}

// ---- one packer for the by-value descriptor tables (GrayTable, RectTable, DepthRegTable, ClaheTable, StateTable) ------------------------------------------------
// blockIdx.y is the descriptor and the grid's x extent follows the largest one (the caller keeps that maximum and clears it in `launch`).
// THE RULE: add(k) flushes first when the next sequence's k descriptors do not fit; flush() sends what is left; launch(tab, n, first) is told whether it
// is the step's first launch -- the one its profile slot times, later ones go out untimed.  The launches are the ones four hand-written loops made:
// colour flushed before adding (n + eyes > GRAY_PACK), as here; rectify flushed after adding at n == RECT_PACK, and with n always even and k == 2 that is
// "the next pair does not fit", sent one add later or by flush(); depth (k == 1) opened a table at n == DEPTHREG_PACK and state cut chunks of STATE_PACK.
template <typename Table, typename Desc, int CAP, typename Launch>
struct TablePacker {
    Table tab;
    Desc (Table::*slots)[CAP];
    Launch launch;
    int n = 0;
    bool first = true;
    TablePacker(Desc (Table::*a)[CAP], Launch l) : slots(a), launch(l) { std::memset(&tab, 0, sizeof(tab)); }
    Desc *add(int k) {
        if (n + k > CAP) flush();
        Desc *d = &(tab.*slots)[n];
        n += k;
        return d;
    }
    void flush() {
        if (n) launch(tab, n, first), first = false, n = 0;
    }
};
// a table's launch on the feature stream: timed by `slot` when it is the step's first
#define LAUNCH_TABLE(first, slot, kern, grid, tab)                          \
    do {                                                                    \
        if (first) LAUNCH(slot, c->stream_f, kern, grid, dim3(256), 0, tab); \
        else hipLaunchKernelGGL(kern, grid, dim3(256), 0, c->stream_f, tab); \
    } while (0)

// ---- one frame for the filters behind the gather (k_depth_guard, k_mask_features) ---------------------------------------------------------------------------
// EVERY sequence of the step takes a slot (slot k of a launch is sequence z0 + k): fill(s, slot) writes sequence s's record and says whether the filter is on
// for it in this step.  The slot is cleared first -- the packer's table is zeroed once, at its construction, and after a flush slot k still holds the record of
// the sequence CAP places before --, so a sequence that is off leaves at the kernel's top.  A table none of whose sequences is on is not launched; the first
// one launched is the step's timed one: launch(tab, n, z0, timed_first).  Returns whether anything was launched (the step's ring flag).
template <typename Table, typename Desc, int CAP, typename Fill, typename Launch>
static bool filter_gathered(Desc (Table::*slots)[CAP], int Bz, Fill fill, Launch launch) {
    int z0 = 0;
    bool any = false, timed = false;
    TablePacker pk(slots, [&](const Table &tab, int n, bool) {
        if (any) launch(tab, n, z0, !timed);
        timed = timed || any;
        z0 += n, any = false;
    });
    for (int s = 0; s < Bz; s++) {
        Desc &d = *pk.add(1);
        d = Desc{};
        any = fill(s, d) || any;
    }
    pk.flush();
    return timed;
}
// a filter's launch on the feature stream, a workgroup of 1024 threads per grid cell: timed by `slot` when it is the step's first
#define LAUNCH_FILTER(first, slot, kern, grid, tab, z0)                                              \
    do {                                                                                             \
        if (first) LAUNCH(slot, c->stream_f, kern, grid, dim3(1024), 0, c->d_seqs, tab, par, z0);    \
        else hipLaunchKernelGGL(kern, grid, dim3(1024), 0, c->stream_f, c->d_seqs, tab, par, z0);    \
    } while (0)

// ---- colour frames: a pixel format per handle / per sequence of a batch (Context::pixfmt) ------------------------------------------------------------
// Every colour image of the step -- both eyes of a stereo sequence, the one image of an RGB-D sequence -- in one launch, AHEAD of the rectify block
// (convert, then remap: the reference's order).  The gray planes (parity `par`) were read last by the feature stage of frame enq - NPAR (k_rectify_frames or
// k_score, k_gather, k_brief_img: all on this stream, all enqueued before), and the source was written by a pull on this stream or belongs to the
// caller: stream order alone covers the hand-over, no gate.
static void convert_colour_frames(Context *c, int slot, int par, int Bz) {
    FrameArgs *fw = &frame_args(c, slot);
    int words = 0;
    TablePacker pk(&GrayTable::im, [&](const GrayTable &tab, int n, bool first) {
        LAUNCH_TABLE(first, 14, k_gray_frames, dim3((words + 255) / 256, n), tab);
        words = 0;
    });
    for (int s = 0; s < Bz; s++) {
        if (c->fmt_of(s) == PIX_GRAY8 || fw[s].absent) continue;
        const int fW = c->frame_W(s), fH = c->frame_H(s);  // (the frame's size: a raw frame's where rectifiers of another source size follow)
        const int dpitch = c->frame_pitch(s), eyes = (c->sensor == 2) ? 1 : 2;
        GrayImg *im = pk.add(eyes);
        for (int e = 0; e < eyes; e++) {
            GrayImg &I = im[e];
            I.src = fw[s].img[e], I.src_pitch = fw[s].img_pitch;
            I.dst = c->d_gray[((size_t)s * NPAR + par) * 2 + e], I.dst_pitch = dpitch;
            I.w = fW, I.h = fH, I.fmt = c->fmt_of(s);
            words = std::max(words, dpitch / 4 * fH);
            fw[s].img[e] = I.dst;
        }
        if (eyes == 1) fw[s].img[1] = fw[s].img[0];
        fw[s].img_pitch = dpitch;
        if (s == 0) c->ring_converted[slot] = true;
    }
    pk.flush();
}
// sequence seq's converted planes hold a frame of its present size (frame_pitch x frame_H): allocated at their first use, and again when the frame has grown
// or shrunk since (rectifiers of another source size attached or detached; no frame is in flight then)
static void give_gray_planes(Context *c, int seq) {
    const int eyes = c->sensor == 2 ? 1 : 2;
    const size_t bytes = (size_t)c->frame_pitch(seq) * c->frame_H(seq) + 64;
    if (c->d_gray.empty()) c->d_gray.assign((size_t)c->B * NPAR * 2, nullptr);
    if (c->gray_bytes.empty()) c->gray_bytes.assign((size_t)c->B, 0);
    if (c->gray_bytes[(size_t)seq] == bytes) return;
    for (int par = 0; par < NPAR; par++)
        for (int e = 0; e < eyes; e++) {
            uint8_t *&d = c->d_gray[((size_t)seq * NPAR + par) * 2 + e];
            c->dfree(d);
            d = c->dalloc<uint8_t>(bytes);
        }
    c->gray_bytes[(size_t)seq] = bytes;
}
static int set_pixel_format(lvt_handle h, int seq, bool batch_call, int format) {
    static const PropertyCall call = {"lvt_amd_set_pixel_format", 0,
                                      {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                       "a batch handle takes its pixel formats per sequence through lvt_amd_batch_set_pixel_format (nothing was changed)"},
                                      "lvt_amd_batch_set_pixel_format on a handle that is not a batch (use lvt_amd_set_pixel_format)"};
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (format < PIX_GRAY8 || format > PIX_RGBA8) return refuse_unchanged(t, call.who, "unknown pixel format " + std::to_string(format));
        if (format != PIX_GRAY8 && c->has_sensor(seq)) return refuse_unchanged(t, call.who, "a colour pixel format on a sequence with a sensor format: a frame is one or the other (unset it first: lvt_amd_set_sensor_format, format LVT_AMD_SENSOR_NONE)");
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the format before the first frame or after every frame has been collected");
        if (format == c->fmt_of(seq)) return 0;
        if (format != PIX_GRAY8) give_gray_planes(c, seq);
        if (seq == 0 && pix_bpp(format) != c->bpp_of(0)) stage_release(c);  // (the pinned staging of the host entry points is sized by bpp: reserved again at the next frame)
        c->n_colour = put_seq_value(c, c->pixfmt, 1, (int)PIX_GRAY8, seq, {format}, [](int f) { return f != PIX_GRAY8; });
        return 0;
    });
}

// ---- sensor formats: Bayer, YUV 4:2:2, 16-bit gray per handle / per sequence of a batch (Context::sens, k_sensor.hip) -------------------------------------
// "" when the record passes on a sequence whose frames are fW x fH: names the offending field and its limits otherwise
static std::string sensor_format_check(const lvt_amd_sensor_format &f, int fW, int fH) {
    if (f.format == SENSOR_NONE) return "";
    if (!sensor_known(f.format)) return "unknown sensor format " + std::to_string(f.format);
    if (f.format == SENSOR_MONO16) {
        if (f.auto_window < 0 || f.auto_window > 1) return "a MONO16 format with auto_window = " + std::to_string(f.auto_window) + " (0 ... 1)";
        if (!f.auto_window) {
            if (f.lo < 0 || f.lo > 65534) return "a MONO16 window with lo = " + std::to_string(f.lo) + " (0 ... 65534)";
            if (f.hi <= f.lo || f.hi > 65535) return "a MONO16 window with hi = " + std::to_string(f.hi) + " (lo + 1 ... 65535)";
        } else {
            if (f.lo_permille < 0 || f.lo_permille > 499) return "a MONO16 auto window with lo_permille = " + std::to_string(f.lo_permille) + " (0 ... 499)";
            if (f.hi_permille < 0 || f.hi_permille > 499) return "a MONO16 auto window with hi_permille = " + std::to_string(f.hi_permille) + " (0 ... 499)";
            if (f.min_span < 1 || f.min_span > 65535) return "a MONO16 auto window with min_span = " + std::to_string(f.min_span) + " (1 ... 65535)";
        }
    }
    if (sensor_is_bayer(f.format)) {
        if (fW < 2) return "a Bayer format on frames of width = " + std::to_string(fW) + " (2 or more)";
        if (fH < 2) return "a Bayer format on frames of height = " + std::to_string(fH) + " (2 or more)";
    }
    return "";
}
// one image's descriptor (win / hist: the auto window's two buffers, nullptr for every other record)
static SensorImg sensor_img(const lvt_amd_sensor_format &f, const uint8_t *src, int src_pitch, int w, int h, uint8_t *dst, int dst_pitch, const int *win, uint32_t *hist) {
    SensorImg I{};
    I.src = src, I.dst = dst, I.win = win, I.hist = hist, I.src_pitch = src_pitch, I.dst_pitch = dst_pitch, I.w = w, I.h = h, I.fmt = f.format;
    I.lo = f.lo, I.hi = f.hi, I.lo_pm = f.lo_permille, I.hi_pm = f.hi_permille, I.min_span = f.min_span;
    return I;
}
static dim3 sensor_hist_grid(int pixels2, int n) {
    const int per = SENSOR_HIST_THREADS * SENSOR_HIST_WORDS;
    return dim3((unsigned)((pixels2 + per - 1) / per), (unsigned)n);
}
// Every image of every sequence that has a sensor format and a frame in this step -- both eyes of a stereo sequence, the one image of an RGB-D sequence -- in
// one launch, in k_gray_frames' place: AHEAD of the reduce, rectify and equalise blocks and of the buffer gate.  The ordering argument is the colour
// formats': the gray planes (parity `par`) were read last by the feature stage of frame enq - NPAR (k_reduce_frames, k_rectify_frames, k_clahe_*, or
// k_score, k_gather, k_brief_img: all on this stream, all enqueued before), and the source was written by a pull on this stream or belongs to the caller:
// stream order alone covers the hand-over, no gate.  The auto window's launches come first, on the same stream: k_sensor_hist adds into bins that
// k_sensor_levels of the frame before left zero (same stream, enqueued before), k_sensor_levels writes the step's windows into this ring slot's record,
// which k_sensor_frames behind it reads and which nothing writes again before the slot is reused, RING frames later, behind this frame's collection.
static void convert_sensor_frames(Context *c, int slot, int par, int Bz) {
    FrameArgs *fw = &frame_args(c, slot);
    const int eyes = (c->sensor == 2) ? 1 : 2;
    if (!c->sens_mapped.empty()) std::fill_n(c->sens_mapped.begin() + (size_t)slot * c->B, (size_t)c->B, (uint8_t)0);
    auto win_of = [&](int s, int e) -> int * { return c->has_sensor_auto(s) ? c->d_sens_win + (((size_t)slot * c->B + s) * 2 + e) * 2 : nullptr; };
    auto img_of = [&](int s, int e) {
        return sensor_img(c->sens[(size_t)s], fw[s].img[e], fw[s].img_pitch, c->frame_W(s), c->frame_H(s), c->d_gray[((size_t)s * NPAR + par) * 2 + e], c->frame_pitch(s), win_of(s, e),
                          c->has_sensor_auto(s) ? c->d_sens_hist[(size_t)s] + (size_t)e * SENSOR_BINS : nullptr);
    };
    if (c->n_sensor_auto) {
        int words = 0;
        TablePacker pk(&SensorTable::im, [&](const SensorTable &tab, int n, bool first) {
            if (first) {
                LAUNCH(31, c->stream_f, k_sensor_hist, sensor_hist_grid(words, n), dim3(SENSOR_HIST_THREADS), 0, tab);
                LAUNCH(32, c->stream_f, k_sensor_levels, dim3(n), dim3(256), 0, tab);
            } else {
                hipLaunchKernelGGL(k_sensor_hist, sensor_hist_grid(words, n), dim3(SENSOR_HIST_THREADS), 0, c->stream_f, tab);
                hipLaunchKernelGGL(k_sensor_levels, dim3(n), dim3(256), 0, c->stream_f, tab);
            }
            words = 0;
        });
        for (int s = 0; s < Bz; s++) {
            if (!c->has_sensor_auto(s) || fw[s].absent) continue;
            SensorImg *im = pk.add(eyes);
            for (int e = 0; e < eyes; e++) {
                im[e] = img_of(s, e);
                words = std::max(words, (im[e].w + 1) / 2 * im[e].h);
            }
        }
        pk.flush();
    }
    int words = 0;
    TablePacker pk(&SensorTable::im, [&](const SensorTable &tab, int n, bool first) {
        LAUNCH_TABLE(first, 30, k_sensor_frames, dim3((words + 255) / 256, n), tab);
        words = 0;
    });
    for (int s = 0; s < Bz; s++) {
        if (!c->has_sensor(s) || fw[s].absent) continue;
        SensorImg *im = pk.add(eyes);
        for (int e = 0; e < eyes; e++) {
            im[e] = img_of(s, e);
            words = std::max(words, im[e].dst_pitch / 4 * im[e].h);
        }
        for (int e = 0; e < eyes; e++) fw[s].img[e] = im[e].dst;
        if (eyes == 1) fw[s].img[1] = fw[s].img[0];
        fw[s].img_pitch = c->frame_pitch(s);
        if (s == 0) c->ring_converted[slot] = true;
        if (c->sens[(size_t)s].format == SENSOR_MONO16) c->sens_mapped[(size_t)slot * c->B + s] = 1;
    }
    pk.flush();
}
// sequence seq's converted planes go back (its sensor format was unset: nothing else uses them, a colour format and a sensor format exclude each other)
static void take_gray_planes(Context *c, int seq) {
    if (c->d_gray.empty() || c->gray_bytes[(size_t)seq] == 0) return;
    for (int par = 0; par < NPAR; par++)
        for (int e = 0; e < 2; e++) {
            uint8_t *&d = c->d_gray[((size_t)seq * NPAR + par) * 2 + e];
            c->dfree(d);
            d = nullptr;
        }
    c->gray_bytes[(size_t)seq] = 0;
}
static int set_sensor_format(lvt_handle h, int seq, bool batch_call, const lvt_amd_sensor_format *f) {
    static const PropertyCall call = {"lvt_amd_set_sensor_format", 0,
                                      {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                       "a batch handle takes its sensor formats per sequence through lvt_amd_batch_set_sensor_format (nothing was changed)"},
                                      "lvt_amd_batch_set_sensor_format on a handle that is not a batch (use lvt_amd_set_sensor_format)"};
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (!f) return refuse_unchanged(t, call.who, "a NULL record (format LVT_AMD_SENSOR_NONE unsets a sensor format)");
        const std::string why = sensor_format_check(*f, c->frame_W(seq), c->frame_H(seq));
        if (!why.empty()) return refuse_unchanged(t, call.who, why);
        const bool on = f->format != SENSOR_NONE;
        if (on && c->fmt_of(seq) != PIX_GRAY8)
            return refuse_unchanged(t, call.who, "a sensor format on a sequence with a colour pixel format: a frame is one or the other (return it to LVT_AMD_PIX_GRAY8 first: lvt_amd_set_pixel_format)");
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the sensor format before the first frame or after every frame has been collected");
        if (!on && !c->has_sensor(seq)) return 0;
        lvt_amd_sensor_format rec = on ? *f : lvt_amd_sensor_format{};
        rec.reserved[0] = 0;
        if (seq == 0) {  // (the host entry points' staging and planes are sized by the frame's bytes; the last frame went in under ANOTHER record)
            frame_planes_release(c);
            std::fill(std::begin(c->ring_converted), std::end(c->ring_converted), false);
        }
        c->n_sensor = put_seq_value(c, c->sens, 1, lvt_amd_sensor_format{}, seq, {rec}, [](const lvt_amd_sensor_format &x) { return x.format != SENSOR_NONE; });
        c->n_sensor_auto = 0;
        for (int s = 0; s < c->B; s++) c->n_sensor_auto += c->has_sensor_auto(s) ? 1 : 0;
        if (c->sens_mapped.empty()) c->sens_mapped.assign((size_t)RING * c->B, 0);
        std::fill(c->sens_mapped.begin(), c->sens_mapped.end(), (uint8_t)0);
        if (on) give_gray_planes(c, seq);
        else take_gray_planes(c, seq);
        if (c->d_sens_hist.empty()) c->d_sens_hist.assign((size_t)c->B, nullptr);
        uint32_t *&hist = c->d_sens_hist[(size_t)seq];
        if (c->has_sensor_auto(seq)) {
            if (!hist) hist = c->dalloc<uint32_t>((size_t)2 * SENSOR_BINS);
            if (!c->d_sens_win) c->d_sens_win = c->dalloc<int>((size_t)RING * c->B * 4);
        } else {
            c->dfree(hist), hist = nullptr;
            if (c->n_sensor_auto == 0) c->dfree(c->d_sens_win), c->d_sens_win = nullptr;
        }
        return 0;
    });
}
// the window image `eye` of sequence seq was mapped with in the last collected frame
static int get_sensor_window(lvt_handle h, int seq, int eye, int *lo, int *hi) {
    h = resolve_handle(h);
    if (is_slot(h)) return (seq == 0 && (eye == 0 || eye == 1)) ? 0 : -1;
    if (!is_ctx(h)) return -1;
    Context *c = static_cast<Context *>(h);
    if (seq < 0 || seq >= c->B || eye < 0 || eye > (c->sensor == 2 ? 0 : 1)) return -1;
    DeviceGuard guard(c);
    try {
        // (frames that are still in flight stay in flight: the LAST COLLECTED frame's record is read, and its k_sensor_levels has run -- the frame was collected.
        //  A synchronous call's frame whose pose has been returned is nobody's to collect: it is drained, as in frames_in_flight)
        if (c->early_pending) drain(c);
        if (c->done == 0 || !c->has_sensor(seq) || c->sens[(size_t)seq].format != SENSOR_MONO16 || !c->sens_mapped[(size_t)c->last_slot * c->B + seq]) return 0;
        int w[2] = {c->sens[(size_t)seq].lo, c->sens[(size_t)seq].hi};
        if (c->has_sensor_auto(seq)) HIPCHK(c, hipMemcpy(w, c->d_sens_win + (((size_t)c->last_slot * c->B + seq) * 2 + eye) * 2, sizeof(w), hipMemcpyDeviceToHost));
        if (lo) *lo = w[0];
        if (hi) *hi = w[1];
        return 1;
    } catch (...) {
    }
    return -1;
}

// ---- large frames: a reduction per handle / per sequence of a batch (Context::red, k_reduce.hip) -------------------------------------------------------
// "" when the record passes on a sequence whose base size is bW x bH: names the offending field and its limits otherwise
static std::string reduction_check(const lvt_amd_reduction &r, int bW, int bH) {
    if (r.factor < 1 || r.factor > REDUCE_MAX_FACTOR) return "a reduction with factor = " + std::to_string(r.factor) + " (1 ... 8)";
    if (r.width < 1 || r.width > REDUCE_MAX_SIDE) return "a reduction with width = " + std::to_string(r.width) + " (1 ... 16384)";
    if (r.height < 1 || r.height > REDUCE_MAX_SIDE) return "a reduction with height = " + std::to_string(r.height) + " (1 ... 16384)";
    if (r.factor >= 2 && (r.width / r.factor != bW || r.height / r.factor != bH))
        return "a frame of " + std::to_string(r.width) + " x " + std::to_string(r.height) + " reduced by " + std::to_string(r.factor) + " is " + std::to_string(r.width / r.factor) + " x " +
               std::to_string(r.height / r.factor) + ", the sequence takes " + std::to_string(bW) + " x " + std::to_string(bH);
    return "";
}
// one image's descriptor: a gray frame (any address, any pitch >= f w) reduced by f into the w x h plane dst
static ReduceImg reduce_img(const uint8_t *src, int src_pitch, int f, uint8_t *dst, int dst_pitch, int w, int h) {
    ReduceImg I{};
    I.src = src, I.dst = dst, I.src_pitch = src_pitch, I.dst_pitch = dst_pitch, I.w = w, I.h = h, I.f = f;
    return I;
}
static dim3 reduce_grid(int words, int n) { return dim3((unsigned)((words + REDUCE_THREADS - 1) / REDUCE_THREADS), (unsigned)n); }
// Every image of every sequence that has a reduction and a frame in this step -- both eyes of a stereo sequence, the one image of an RGB-D sequence -- in one
// launch, BEHIND the conversion (a colour frame is averaged as the gray image it converts to) and AHEAD of the rectify block (the rectifiers' source is the
// reduced image).  The reduced planes (parity `par`) were read last by the feature stage of frame enq - NPAR (k_rectify_frames, k_clahe_*, or k_score,
// k_gather, k_brief_img: all on this stream, all enqueued before), and the source was written on this stream (a pull, k_gray_frames) or belongs to the
// caller: stream order alone covers the hand-over, no gate.
static void reduce_frames(Context *c, int slot, int par, int Bz) {
    FrameArgs *fw = &frame_args(c, slot);
    int words = 0;
    TablePacker pk(&ReduceTable::im, [&](const ReduceTable &tab, int n, bool first) {
        if (first) LAUNCH(29, c->stream_f, k_reduce_frames, reduce_grid(words, n), dim3(REDUCE_THREADS), 0, tab);
        else hipLaunchKernelGGL(k_reduce_frames, reduce_grid(words, n), dim3(REDUCE_THREADS), 0, c->stream_f, tab);
        words = 0;
    });
    for (int s = 0; s < Bz; s++) {
        if (!c->has_reduce(s) || fw[s].absent) continue;
        const int bW = c->base_W(s), bH = c->base_H(s), dpitch = c->base_pitch(s), eyes = (c->sensor == 2) ? 1 : 2;
        ReduceImg *im = pk.add(eyes);
        for (int e = 0; e < eyes; e++) {
            im[e] = reduce_img(fw[s].img[e], fw[s].img_pitch, c->red[(size_t)s].factor, c->d_red[((size_t)s * NPAR + par) * 2 + e], dpitch, bW, bH);
            words = std::max(words, dpitch / 4 * bH);
            fw[s].img[e] = im[e].dst;
        }
        if (eyes == 1) fw[s].img[1] = fw[s].img[0];
        fw[s].img_pitch = dpitch;
        if (s == 0) c->ring_reduced[slot] = true;
    }
    pk.flush();
}
// sequence seq's reduced planes hold an image of its base size (base_pitch x base_H): allocated at the set, again when the base has changed since, and given
// back (on == false) when the reduction is cleared; no frame is in flight then
static void give_red_planes(Context *c, int seq, bool on) {
    const int eyes = c->sensor == 2 ? 1 : 2;
    const size_t bytes = on ? (size_t)c->base_pitch(seq) * c->base_H(seq) + 64 : 0;
    if (c->d_red.empty()) c->d_red.assign((size_t)c->B * NPAR * 2, nullptr);
    if (c->red_bytes.empty()) c->red_bytes.assign((size_t)c->B, 0);
    if (c->red_bytes[(size_t)seq] == bytes) return;
    for (int par = 0; par < NPAR; par++)
        for (int e = 0; e < eyes; e++) {
            uint8_t *&d = c->d_red[((size_t)seq * NPAR + par) * 2 + e];
            c->dfree(d);
            d = bytes ? c->dalloc<uint8_t>(bytes) : nullptr;
        }
    c->red_bytes[(size_t)seq] = bytes;
}
static int set_reduction(lvt_handle h, int seq, bool batch_call, const lvt_amd_reduction *r) {
    static const PropertyCall call = {"lvt_amd_set_reduction", 0,
                                      {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                       "a batch handle takes its reductions per sequence through lvt_amd_batch_set_reduction (nothing was changed)"},
                                      "lvt_amd_batch_set_reduction on a handle that is not a batch (use lvt_amd_set_reduction)"};
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (!r) return refuse_unchanged(t, call.who, "a NULL record (factor 1 clears a reduction)");
        const std::string why = reduction_check(*r, c->base_W(seq), c->base_H(seq));
        if (!why.empty()) return refuse_unchanged(t, call.who, why);
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the reduction before the first frame or after every frame has been collected");
        const bool on = r->factor >= 2;
        if (!on && !c->has_reduce(seq)) return 0;
        if (seq == 0) std::fill(std::begin(c->ring_reduced), std::end(c->ring_reduced), false);  // (the last frame went in under ANOTHER record: lvt_amd_get_plane(.., 9, ..) has nothing of it)
        const int fW = c->frame_W(seq), fH = c->frame_H(seq);
        c->n_reduce = put_seq_value(c, c->red, 1, lvt_amd_reduction{}, seq, {on ? *r : lvt_amd_reduction{}}, [](const lvt_amd_reduction &x) { return x.factor >= 2; });
        give_red_planes(c, seq, on);
        if (c->frame_W(seq) != fW || c->frame_H(seq) != fH) {  // the frame's size changed: what is sized by its bytes follows, as in set_rectifiers
            if (seq == 0) frame_planes_release(c);
            if (c->converts(seq)) give_gray_planes(c, seq);
        }
        return 0;
    });
}

// ---- raw frames: rectifiers attached to a tracker (Context::rect) -----------------------------------------------------------------------------------
// Both eyes of every sequence that has rectifiers and a frame in this step, in one launch.  The rectified planes (parity `par`) were read last by the
// feature stage of frame enq - NPAR -- k_score, k_gather, k_brief_img: all on this stream, all enqueued before -- so stream order alone covers the
// hand-over, and the launch needs no gate: it goes out ahead of the buffer gate.
static void rectify_raw_frames(Context *c, int slot, int par, int Bz) {
    FrameArgs *fw = &frame_args(c, slot);
    int words = 0;
    TablePacker pk(&RectTable::im, [&](const RectTable &tab, int n, bool first) {
        LAUNCH_TABLE(first, 4, k_rectify_frames, dim3((words + 255) / 256, n), tab);
        words = 0;
    });
    for (int s = 0; s < Bz; s++) {
        if (!c->has_rect(s) || fw[s].absent) continue;
        const Params &q = c->seq_prm(s);
        const int dpitch = c->h_seqs[s].plane_pitch;
        const Rectifier *r0 = c->rect[2 * (size_t)s];
        RectImg *im = pk.add(2);
        for (int e = 0; e < 2; e++) {
            RectImg &I = im[e];
            I.src = fw[s].img[e], I.src_pitch = fw[s].img_pitch;
            I.map = c->rect[2 * (size_t)s + e]->d_fix;
            I.dst = c->d_rect[((size_t)s * NPAR + par) * 2 + e], I.dst_pitch = dpitch;
            I.sw = r0->sw, I.sh = r0->sh, I.dw = q.W, I.dh = q.H;  // (the source: the lens's size, the same for both eyes; the destination: the sequence's)
            words = std::max(words, dpitch / 4 * q.H);
            fw[s].img[e] = I.dst;
        }
        fw[s].img_pitch = dpitch;
    }
    pk.flush();
}
// (the batch spelling on a solo handle is accepted for seq == 0)
static int set_rectifiers(lvt_handle h, int seq, bool batch_call, lvt_amd_rectifier left, lvt_amd_rectifier right) {
    static const PropertyCall call = {"lvt_amd_set_rectifiers", 1,
                                      {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)",
                                       "an RGB-D handle (there is one image, and its depth plane is registered to it) (nothing was changed)",
                                       "a batch handle takes its rectifiers per sequence through lvt_amd_batch_set_rectifiers (nothing was changed)"},
                                      nullptr};
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (c->has_reduce(seq))  // (the reduction was checked against THIS base size: rectifiers first, then the reduction)
            return refuse_unchanged(t, call.who, "a sequence with a reduction in force: clear it first (lvt_amd_set_reduction, factor 1), attach or detach, then set it again");
        if ((left == nullptr) != (right == nullptr)) return refuse_unchanged(t, call.who, "one rectifier is NULL (both, or NULL, NULL to detach)");
        Rectifier *rl = static_cast<Rectifier *>(left), *rr = static_cast<Rectifier *>(right);
        const Params &q = c->seq_prm(seq);
        for (Rectifier *r : {rl, rr}) {
            if (!r) continue;
            if (r->w != q.W || r->h != q.H)  // (its DESTINATION: what it writes is what the sequence tracks)
                return refuse_unchanged(t, call.who, "a rectifier of " + std::to_string(r->w) + " x " + std::to_string(r->h) + " on a sequence of " + std::to_string(q.W) + " x " + std::to_string(q.H));
            if (r->device != c->device)
                return refuse_unchanged(t, call.who, "a rectifier created on device " + std::to_string(r->device) + ", the handle owns device " + std::to_string(c->device));
        }
        if (rl && (rl->sw != rr->sw || rl->sh != rr->sh))  // (one frame size per sequence: both eyes arrive through one n_rows x n_cols)
            return refuse_unchanged(t, call.who, "the left rectifier's source is " + std::to_string(rl->sw) + " x " + std::to_string(rl->sh) + ", the right one's " + std::to_string(rr->sw) + " x " + std::to_string(rr->sh) + ": a sequence's two raw images have one size");
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: attach before the first frame or after every frame has been collected");
        if (rl) give_planes(c, c->d_rect, 2, seq, 2, 64);
        const int fW = c->frame_W(seq), fH = c->frame_H(seq);
        c->n_rect = put_seq_value(c, c->rect, 2, (Rectifier *)nullptr, seq, {rl, rr}, [](const Rectifier *r) { return r != nullptr; });
        if (c->frame_W(seq) != fW || c->frame_H(seq) != fH) {  // the frame's size changed: what is sized by its bytes follows (a same-size attach: nothing)
            if (seq == 0) frame_planes_release(c);
            if (c->converts(seq)) give_gray_planes(c, seq);
        }
        return 0;
    });
}

// ---- unregistered depth: a depth camera per handle / per sequence of a batch (Context::depth_cam, k_depthreg.hip) --------------------------------------
// "" when the record passes
static std::string depth_camera_check(const lvt_amd_depth_camera &d) {
    if (d.width < 1 || d.width > 8192 || d.height < 1 || d.height > 8192)
        return "a depth camera of " + std::to_string(d.width) + " x " + std::to_string(d.height) + " pixels (1 ... 8192 each way)";
    bool finite = std::isfinite(d.fx) && std::isfinite(d.fy) && std::isfinite(d.cx) && std::isfinite(d.cy);
    for (float v : d.R) finite = finite && std::isfinite(v);
    for (float v : d.t) finite = finite && std::isfinite(v);
    if (!finite) return "a depth camera with a non-finite field";
    if (!(d.fx > 0.f && d.fy > 0.f)) return "a depth camera whose fx or fy is not > 0";
    return "";
}
// one depth plane's descriptor: the sensor's plane (src_pitch in ELEMENTS of fmt; scale only for DEPTH_U16) registered to the colour camera's pixel grid in dst
static DepthRegImg depth_reg_img(const lvt_amd_depth_camera &dc, const lvt_amd_params &q, const void *src, int src_pitch, int fmt, float scale, float *dst, int dst_pitch) {
    DepthRegImg I{};
    I.src = src, I.src_pitch = src_pitch, I.fmt = fmt, I.scale = (fmt == DEPTH_U16) ? scale : 0.f;
    I.dst = dst, I.dst_pitch = dst_pitch;
    I.dw = dc.width, I.dh = dc.height, I.fx = dc.fx, I.fy = dc.fy, I.cx = dc.cx, I.cy = dc.cy;
    std::memcpy(I.R, dc.R, sizeof(I.R)), std::memcpy(I.t, dc.t, sizeof(I.t));
    I.cfx = q.fx, I.cfy = q.fy, I.ccx = q.cx, I.ccy = q.cy, I.k1 = q.k1, I.k2 = q.k2, I.p1 = q.p1, I.p2 = q.p2, I.k3 = q.k3;
    I.W = q.img_width, I.H = q.img_height;
    return I;
}
// Every sequence that has a depth camera and a frame in this step.  The descriptors are built HERE, on the host, and the frame is pointed at the sequence's
// registered plane before k_score<true> / k_feat_begin* carries the record into FeatCtl::in; k_depth_clear goes out now, k_depth_register directly in front
// of k_gather (scatter_depth_planes).  The registered plane (parity `par`) was read last by k_gather of frame enq - NPAR -- on this stream, enqueued before --
// and the source was written by a pull this stream waits for or belongs to the caller: stream order alone covers the hand-over, no gate.
// Both kernels take each table, so the step keeps them (DepthRegPlan: the first in place, only a step with more than DEPTHREG_PACK registered sequences
// takes tables from the heap).
static void begin_depth_registration(Context *c, int slot, int par, int Bz, DepthRegPlan &plan) {
    FrameArgs *fw = &frame_args(c, slot);
    int px = 0, words = 0;
    TablePacker pk(&DepthRegTable::im, [&](const DepthRegTable &tab, int n, bool first) {
        LAUNCH_TABLE(first, 17, k_depth_clear, dim3(((words + 3) / 4 + 255) / 256, n), tab);
        DepthRegStep &T = first ? plan.first : (plan.more.emplace_back(), plan.more.back());
        T.tab = tab, T.n = n, T.px = px;
        plan.n++, px = 0, words = 0;
    });
    for (int s = 0; s < Bz; s++) {
        if (!c->has_depth_cam(s) || fw[s].absent) continue;
        const lvt_amd_depth_camera &dc = c->depth_cam[(size_t)s];
        DepthRegImg &I = *pk.add(1);
        I = depth_reg_img(dc, c->in_prms[c->mixed ? (size_t)s : 0], fw[s].depth, fw[s].depth_pitch, fw[s].depth_format, fw[s].depth_scale, c->d_reg[(size_t)s * NPAR + par],
                          c->h_seqs[s].plane_pitch);
        px = std::max(px, dc.width * dc.height), words = std::max(words, I.dst_pitch * I.H);
        fw[s].depth = I.dst, fw[s].depth_pitch = I.dst_pitch, fw[s].depth_format = DEPTH_F32, fw[s].depth_scale = 0.f;
        if (s == 0) c->ring_registered[slot] = true;
    }
    pk.flush();
}
// the z-buffered scatter of the step's unregistered depth planes (a host call's depth plane arrives on the early stream: the caller has waited for ev_depth)
static void scatter_depth_planes(Context *c, const DepthRegPlan &plan) {
    for (int k = 0; k < plan.n; k++) {
        const DepthRegStep &T = k == 0 ? plan.first : plan.more[(size_t)k - 1];
        LAUNCH_TABLE(k == 0, 21, k_depth_register, dim3((T.px + 255) / 256, T.n), T.tab);
    }
}
static int set_depth_camera(lvt_handle h, int seq, bool batch_call, const lvt_amd_depth_camera *cam) {
    static const PropertyCall call = {"lvt_amd_set_depth_camera", 2,
                                      {"a pooled handle (pooled handles are stereo only) (nothing was changed)",
                                       "a stereo handle (it has no depth plane to register) (nothing was changed)",
                                       "a batch handle takes its depth cameras per sequence through lvt_amd_batch_set_depth_camera (nothing was changed)"},
                                      "lvt_amd_batch_set_depth_camera on a handle that is not a batch (use lvt_amd_set_depth_camera)"};
    // (an lvt_create handle is a stereo handle: refused like one)
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (cam) {
            const std::string why = depth_camera_check(*cam);
            if (!why.empty()) return refuse_unchanged(t, call.who, why);
        }
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the camera before the first frame or after every frame has been collected");
        if (!cam && !c->has_depth_cam(seq)) return 0;
        if (cam) give_planes(c, c->d_reg, 1, seq, 1, 16);
        if (seq == 0) stage_release(c);  // (the pinned staging of the host entry points is sized by the depth plane: reserved again at the next frame)
        c->n_depth_cam = put_seq_value(c, c->depth_cam, 1, lvt_amd_depth_camera{}, seq, {cam ? *cam : lvt_amd_depth_camera{}}, [](const lvt_amd_depth_camera &d) { return d.width > 0; });
        return 0;
    });
}

// ---- dim frames: an equalisation record per handle / per sequence of a batch (Context::equal, k_equalise.hip) -----------------------------------------
// steps 1 and 2 of the definition (include/lvt_amd_ext.h) for a w x h image
struct EqualPlan {
    int Wp, Hp, tile_w, tile_h, area, clip;
    float lut_scale;
};
// "" when the record passes on an image of w x h: names the offending field and its limits otherwise
static std::string equalisation_check(const lvt_amd_equalisation &e, int w, int h) {
    if (e.tiles_x < 1 || e.tiles_x > CLAHE_MAX_TILES) return "an equalisation with tiles_x = " + std::to_string(e.tiles_x) + " (1 ... 16)";
    if (e.tiles_y < 1 || e.tiles_y > CLAHE_MAX_TILES) return "an equalisation with tiles_y = " + std::to_string(e.tiles_y) + " (1 ... 16)";
    if (!(std::isfinite(e.clip_limit) && e.clip_limit > 0.f)) return "an equalisation whose clip_limit is not finite and > 0";
    if (e.tiles_x > w) return "an equalisation with tiles_x = " + std::to_string(e.tiles_x) + " on an image " + std::to_string(w) + " pixels wide (tiles_x <= img_width)";
    if (e.tiles_y > h) return "an equalisation with tiles_y = " + std::to_string(e.tiles_y) + " on an image " + std::to_string(h) + " pixels high (tiles_y <= img_height)";
    return "";
}
static EqualPlan equalisation_plan(const lvt_amd_equalisation &e, int w, int h) {
    EqualPlan p;
    p.Wp = w + (e.tiles_x - w % e.tiles_x) % e.tiles_x, p.Hp = h + (e.tiles_y - h % e.tiles_y) % e.tiles_y;
    p.tile_w = p.Wp / e.tiles_x, p.tile_h = p.Hp / e.tiles_y, p.area = p.tile_w * p.tile_h;
    const float fa = (float)p.area;
    const float c = e.clip_limit * fa / 256.0f;  // (two fp32 operations, left to right; may overflow to +inf: then c >= fa)
    p.clip = (c >= fa) ? p.area : std::max((int)c, 1);
    p.lut_scale = 255.0f / fa;
    return p;
}
// one image's descriptor: src (any pitch >= w) equalised into dst with the tables in lut
static ClaheImg clahe_img(const lvt_amd_equalisation &e, const uint8_t *src, int src_pitch, int w, int h, uint8_t *dst, int dst_pitch, uint8_t *lut, int direct) {
    const EqualPlan p = equalisation_plan(e, w, h);
    ClaheImg I{};
    I.src = src, I.dst = dst, I.lut = lut, I.src_pitch = src_pitch, I.dst_pitch = dst_pitch, I.w = w, I.h = h;
    I.tiles_x = e.tiles_x, I.tiles_y = e.tiles_y, I.tile_w = p.tile_w, I.tile_h = p.tile_h, I.clip = p.clip, I.lut_scale = p.lut_scale;
    I.inv_tw = 1.0f / (float)p.tile_w, I.inv_th = 1.0f / (float)p.tile_h, I.direct = direct;
    return I;
}
// LVT_AMD_CLAHE_GATHER=l1: k_clahe_apply gathers its tables through L1 instead of staging them in LDS (tools/equalisation.py measures both)
static int clahe_direct() {
    static const int v = [] {
        const char *e = std::getenv("LVT_AMD_CLAHE_GATHER");
        return (e && std::strcmp(e, "l1") == 0) ? 1 : 0;
    }();
    return v;
}
// Every image of every sequence that has a record and a frame in this step -- both eyes of a stereo sequence, the one image of an RGB-D sequence -- in TWO
// launches per table, behind the conversion and the remap: what is equalised is exactly the plane k_score would have read, and k_gather's box-sum fall-back
// and k_brief_img see the equalised plane too, through FrameIn::img.  The equalised planes (parity `par`) were read last by the feature stage of frame
// enq - NPAR -- k_score, k_gather, k_brief_img: all on this stream, all enqueued before --; the tables were read last by k_clahe_apply of the previous frame,
// on this stream; and the source was written on this stream (a pull, k_gray_frames, k_rectify_frames) or belongs to the caller: stream order alone covers
// the hand-over, and the launches need no gate: they go out ahead of the buffer gate.
static void equalise_frames(Context *c, int slot, int par, int Bz) {
    FrameArgs *fw = &frame_args(c, slot);
    int words = 0, tiles = 0;
    TablePacker pk(&ClaheTable::im, [&](const ClaheTable &tab, int n, bool first) {
        LAUNCH_TABLE(first, 24, k_clahe_lut, dim3(tiles, n), tab);
        LAUNCH_TABLE(first, 25, k_clahe_apply, dim3((words + 255) / 256, n), tab);
        words = 0, tiles = 0;
    });
    for (int s = 0; s < Bz; s++) {
        if (!c->has_equal(s) || fw[s].absent) continue;
        const Params &q = c->seq_prm(s);
        const lvt_amd_equalisation &e = c->equal[(size_t)s];
        const int dpitch = c->h_seqs[s].plane_pitch, eyes = (c->sensor == 2) ? 1 : 2;
        ClaheImg *im = pk.add(eyes);
        for (int k = 0; k < eyes; k++) {
            im[k] = clahe_img(e, fw[s].img[k], fw[s].img_pitch, q.W, q.H, c->d_eq[((size_t)s * NPAR + par) * 2 + k], dpitch, c->d_eq_lut[(size_t)s * 2 + k], clahe_direct());
            words = std::max(words, dpitch / 4 * q.H), tiles = std::max(tiles, e.tiles_x * e.tiles_y);
            fw[s].img[k] = im[k].dst;
        }
        if (eyes == 1) fw[s].img[1] = fw[s].img[0];
        fw[s].img_pitch = dpitch;
        if (s == 0) c->ring_equalised[slot] = true;
    }
    pk.flush();
}
static int set_equalisation(lvt_handle h, int seq, bool batch_call, const lvt_amd_equalisation *cfg) {
    static const PropertyCall call = {"lvt_amd_set_equalisation", 0,
                                      {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                       "a batch handle takes its equalisation per sequence through lvt_amd_batch_set_equalisation (nothing was changed)"},
                                      "lvt_amd_batch_set_equalisation on a handle that is not a batch (use lvt_amd_set_equalisation)"};
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (cfg) {
            const std::string why = equalisation_check(*cfg, c->seq_prm(seq).W, c->seq_prm(seq).H);
            if (!why.empty()) return refuse_unchanged(t, call.who, why);
        }
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the equalisation before the first frame or after every frame has been collected");
        if (!cfg && !c->has_equal(seq)) return 0;
        if (seq == 0) std::fill(std::begin(c->ring_equalised), std::end(c->ring_equalised), false);  // (the last frame went in before THIS record: lvt_amd_get_plane(.., 5 / 6, ..) has nothing of it)
        if (cfg) {
            const int eyes = c->sensor == 2 ? 1 : 2;
            give_planes(c, c->d_eq, 2, seq, eyes, 64);
            if (c->d_eq_lut.empty()) c->d_eq_lut.assign((size_t)c->B * 2, nullptr);
            for (int e = 0; e < eyes; e++)
                if (!c->d_eq_lut[(size_t)seq * 2 + e]) c->d_eq_lut[(size_t)seq * 2 + e] = c->dalloc<uint8_t>((size_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES * 256);
        }
        c->n_equal = put_seq_value(c, c->equal, 1, lvt_amd_equalisation{}, seq, {cfg ? *cfg : lvt_amd_equalisation{}}, [](const lvt_amd_equalisation &e) { return e.tiles_x > 0; });
        return 0;
    });
}

// ---- depth guard: a record per RGB-D handle / per sequence of an RGB-D batch (Context::depth_guard, k_depthguard.hip) ------------------------------------
// "" when the record passes: names the offending field and its limits otherwise
static std::string depth_guard_check(const lvt_amd_depth_guard &g) {
    if (g.radius < 1 || g.radius > 3) return "a depth guard with radius = " + std::to_string(g.radius) + " (1 ... 3)";
    const int most = (2 * g.radius + 1) * (2 * g.radius + 1) - 1;
    if (g.min_support < 1 || g.min_support > most)
        return "a depth guard with min_support = " + std::to_string(g.min_support) + " at radius " + std::to_string(g.radius) + " (1 ... " + std::to_string(most) + ")";
    if (!(std::isfinite(g.tol_abs) && g.tol_abs >= 0.f)) return "a depth guard whose tol_abs is not finite and >= 0";
    if (!(std::isfinite(g.tol_rel) && g.tol_rel >= 0.f)) return "a depth guard whose tol_rel is not finite and >= 0";
    return "";
}
// A sequence without a guard, or without a frame in this step, has radius 0 (filter_gathered).  The launch stands directly behind k_gather and ahead of
// k_mask_features and k_brief / k_brief_img, in both orderings.  The depth plane is the one FeatCtl::in names -- k_gather has just read it on this stream, so
// whatever made it complete for k_gather (the wait for ev_depth, k_depth_register) holds for the guard --, and the Feat arrays are written by k_gather just
// ahead and read just behind, on this stream: stream order alone covers the hand-over, no gate.
static void guard_features(Context *c, int slot, int par, int Bz) {
    const FrameArgs *fw = &frame_args(c, slot);
    c->ring_guarded[slot] = filter_gathered(
        &GuardTable::s, Bz,
        [&](int s, GuardSeq &G) {
            if (!c->has_guard(s) || fw[s].absent) return false;
            const lvt_amd_depth_guard &g = c->depth_guard[(size_t)s];
            G = GuardSeq{g.radius, g.min_support, g.tol_abs, g.tol_rel};
            return true;
        },
        [&](const GuardTable &tab, int n, int z0, bool first) { LAUNCH_FILTER(first, 27, k_depth_guard, dim3(1, 1, n), tab, z0); });
}
static int set_depth_guard(lvt_handle h, int seq, bool batch_call, const lvt_amd_depth_guard *cfg) {
    static const PropertyCall call = {"lvt_amd_set_depth_guard", 2,
                                      {"a pooled handle (pooled handles are stereo only) (nothing was changed)",
                                       "a stereo handle (it has no depth plane to guard) (nothing was changed)",
                                       "a batch handle takes its depth guards per sequence through lvt_amd_batch_set_depth_guard (nothing was changed)"},
                                      "lvt_amd_batch_set_depth_guard on a handle that is not a batch (use lvt_amd_set_depth_guard)"};
    // (an lvt_create handle is a stereo handle: refused like one)
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (cfg) {
            const std::string why = depth_guard_check(*cfg);
            if (!why.empty()) return refuse_unchanged(t, call.who, why);
        }
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the depth guard before the first frame or after every frame has been collected");
        if (!cfg && !c->has_guard(seq)) return 0;
        std::fill(std::begin(c->ring_guarded), std::end(c->ring_guarded), false);  // (the last frame went in under ANOTHER record: lvt_amd_get_depth_guard_stats has nothing of it)
        c->n_guard = put_seq_value(c, c->depth_guard, 1, lvt_amd_depth_guard{}, seq, {cfg ? *cfg : lvt_amd_depth_guard{}}, [](const lvt_amd_depth_guard &g) { return g.radius > 0; });
        return 0;
    });
}

// ---- feature masks: u8 planes per handle / per sequence of a batch, one per eye (Context::d_mask, k_mask.hip) -------------------------------------------
// An eye without a mask, and every eye of a sequence without one or without a frame in this step, is a NULL pointer (filter_gathered).  The launch stands
// directly behind k_gather and ahead of k_brief / k_brief_img, in both orderings.  The planes are written only by a set on a quiet handle, whose copy has
// completed before the set returns; the Feat arrays are written by k_gather just ahead and read by k_brief just behind, on this stream: stream order alone
// covers the hand-over, no gate.
// An eye the step built a label plane for (build_label_masks, below) is handed THAT plane -- it holds the static mask already --; called where n_mask || n_label.
static void mask_features(Context *c, int slot, int par, int Bz) {
    const FrameArgs *fw = &frame_args(c, slot);
    c->ring_masked[slot] = filter_gathered(
        &MaskTable::s, Bz,
        [&](int s, MaskSeq &M) {
            for (int e = 0; e < 2; e++) {
                if (c->built_label(slot, s, e)) M.mask[e] = c->d_lmask[((size_t)s * NPAR + par) * 2 + e];
                else M.mask[e] = c->has_mask(s, e) && !fw[s].absent ? c->d_mask[(size_t)s * 2 + e] : nullptr;
                M.pitch[e] = c->h_seqs[s].plane_pitch;
            }
            return M.mask[0] || M.mask[1];
        },
        [&](const MaskTable &tab, int n, int z0, bool first) { LAUNCH_FILTER(first, 26, k_mask_features, dim3(1, 2, n), tab, z0); });
}
// left / right: tightly packed host planes (device == false: the pitch is the width) or planes in HBM at any address and the given pitch; NULL: that eye has no
// mask; both NULL: the sequence has none
static int set_mask(lvt_handle h, int seq, bool batch_call, bool device, const void *left, int pitch_l, const void *right, int pitch_r) {
    static const PropertyCall host_call = {"lvt_amd_set_mask", 0,
                                           {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                            "a batch handle takes its masks per sequence through lvt_amd_batch_set_mask (nothing was changed)"},
                                           "lvt_amd_batch_set_mask on a handle that is not a batch (use lvt_amd_set_mask)"};
    static const PropertyCall device_call = {"lvt_amd_set_mask_device", 0,
                                             {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                              "a batch handle takes its masks per sequence through lvt_amd_batch_set_mask_device (nothing was changed)"},
                                             "lvt_amd_batch_set_mask_device on a handle that is not a batch (use lvt_amd_set_mask_device)"};
    const PropertyCall &call = device ? device_call : host_call;
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        const Params &q = c->seq_prm(seq);
        const void *src[2] = {left, right};
        const int pitch[2] = {device ? pitch_l : q.W, device ? pitch_r : q.W};
        for (int e = 0; e < 2; e++)
            if (src[e] && pitch[e] < q.W)
                return refuse_unchanged(t, call.who, "a mask pitch of " + std::to_string(pitch[e]) + " bytes on a sequence " + std::to_string(q.W) + " pixels wide (pitch >= img_width)");
        if (right && c->sensor == 2) return refuse_unchanged(t, call.who, "a right-eye mask on an RGB-D handle (it has one image: pass NULL for the right eye)");
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the mask before the first frame or after every frame has been collected");
        if (!left && !right && !(c->has_mask(seq, 0) || c->has_mask(seq, 1))) return 0;
        std::fill(std::begin(c->ring_masked), std::end(c->ring_masked), false);  // (the last frame went in under OTHER masks: lvt_amd_get_mask_stats has nothing of it)
        if (left || right) {
            give_planes(c, c->d_mask, 2, seq, c->sensor == 2 ? 1 : 2, 64, 1);
            // in the order of the handle's tracking stream (the caller's, where lvt_amd_set_stream gave one): a device plane the caller wrote on that stream is
            // complete before it is read, and the copy has completed before the call returns -- no frame's launch can overtake it
            for (int e = 0; e < 2; e++)
                if (src[e])
                    HIPCHK(c, hipMemcpy2DAsync(c->d_mask[(size_t)seq * 2 + e], (size_t)c->h_seqs[seq].plane_pitch, src[e], (size_t)pitch[e], (size_t)q.W, (size_t)q.H,
                                               device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (c->mask_on.empty()) c->mask_on.assign((size_t)c->B * 2, 0);
        c->mask_on[(size_t)seq * 2] = left != nullptr, c->mask_on[(size_t)seq * 2 + 1] = right != nullptr;
        c->n_mask = 0;
        for (int s = 0; s < c->B; s++) c->n_mask += (c->mask_on[(size_t)s * 2] || c->mask_on[(size_t)s * 2 + 1]) ? 1 : 0;
        return 0;
    });
}

// ---- label masks: a record per handle / per sequence of a batch, a label image per eye and FRAME (Context::label, Context::label_ring, k_labelmask.hip) ------
// "" when the record passes: names the offending field and its limits otherwise
static std::string label_mask_check(const lvt_amd_label_mask &r) {
    if (r.label_width < 1 || r.label_width > 8192) return "a label mask with label_width = " + std::to_string(r.label_width) + " (1 ... 8192)";
    if (r.label_height < 1 || r.label_height > 8192) return "a label mask with label_height = " + std::to_string(r.label_height) + " (1 ... 8192)";
    if (r.dilate < 0 || r.dilate > LABEL_MAX_DILATE) return "a label mask with dilate = " + std::to_string(r.dilate) + " (0 ... 15)";
    return "";
}
// one image's descriptor: the label image under record r onto a W x H grid, ANDed with the static mask (or NULL), into dst
static LabelImg label_img(const lvt_amd_label_mask &r, const uint8_t *lab, int lab_pitch, int W, int H, const uint8_t *stat, int stat_pitch, uint8_t *dst, int dst_pitch) {
    LabelImg I{};
    I.lab = lab, I.stat = stat, I.dst = dst;
    I.lab_pitch = lab_pitch, I.lw = r.label_width, I.lh = r.label_height, I.stat_pitch = stat_pitch, I.dst_pitch = dst_pitch, I.W = W, I.H = H, I.dilate = r.dilate;
    for (int l = 0; l < 256; l++)
        if (r.drop[l]) I.drop[l >> 5] |= 1u << (l & 31);
    return I;
}
// workgroups of k_label_mask for a plane of dst_pitch x H: tiles of 32 x 32 over the pitch
static int label_tiles(int dst_pitch, int H) { return ((dst_pitch / 4 + 7) / 8) * ((H + LABEL_TILE - 1) / LABEL_TILE); }
// Every eye of every sequence that has a record, a frame in this step and an attachment TAGGED with this frame's number (enq + 1), in one launch.  An attachment
// with another tag stays where it is: it belongs to a later frame (the one behind a held frame), or to a step long gone, and the next call for that slot
// overwrites it.  The built plane (parity `par`) was read last by k_mask_features of frame enq - NPAR, which was enqueued on this stream earlier; the label source
// was written by lvt_amd_frame_labels' copy on this stream or belongs to the caller (on a caller's stream: behind the step's ev_caller wait); the static mask is
// written only on a quiet handle: stream order alone covers the hand-over, no gate.
static void build_label_masks(Context *c, int slot, int par, int Bz) {
    const FrameArgs *fw = &frame_args(c, slot);
    const long long frame = (long long)c->enq + 1;
    int tiles = 0;
    TablePacker pk(&LabelTable::im, [&](const LabelTable &tab, int n, bool first) {
        LAUNCH_TABLE(first, 28, k_label_mask, dim3(tiles, n), tab);
        tiles = 0;
    });
    for (int s = 0; s < Bz; s++) {
        const Context::LabelAttach &A = c->label_ring[(size_t)slot * c->B + s];
        if (!c->has_label(s) || A.frame != frame || fw[s].absent) continue;
        const Params &q = c->seq_prm(s);
        const int dpitch = c->h_seqs[s].plane_pitch;
        for (int e = 0; e < 2; e++) {
            if (!A.src[e]) continue;
            *pk.add(1) = label_img(c->label[(size_t)s], A.src[e], A.pitch[e], q.W, q.H, c->has_mask(s, e) ? c->d_mask[(size_t)s * 2 + e] : nullptr, dpitch,
                                   c->d_lmask[((size_t)s * NPAR + par) * 2 + e], dpitch);
            tiles = std::max(tiles, label_tiles(dpitch, q.H));
            c->label_built[((size_t)slot * c->B + s) * 2 + e] = 1;
        }
    }
    pk.flush();
}
static int set_label_mask(lvt_handle h, int seq, bool batch_call, const lvt_amd_label_mask *cfg) {
    static const PropertyCall call = {"lvt_amd_set_label_mask", 0,
                                      {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr,
                                       "a batch handle takes its label masks per sequence through lvt_amd_batch_set_label_mask (nothing was changed)"},
                                      "lvt_amd_batch_set_label_mask on a handle that is not a batch (use lvt_amd_set_label_mask)"};
    return set_property(h, call, seq, batch_call, [&](lvt_handle t, Context *c) -> int {
        if (cfg) {
            const std::string why = label_mask_check(*cfg);
            if (!why.empty()) return refuse_unchanged(t, call.who, why);
        }
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: set the label mask before the first frame or after every frame has been collected");
        if (!cfg && !c->has_label(seq)) return 0;
        std::fill(std::begin(c->ring_masked), std::end(c->ring_masked), false);  // (the last frame went in under ANOTHER record: lvt_amd_get_mask_stats has nothing of it)
        if (c->label_ring.empty()) c->label_ring.assign((size_t)RING * c->B, Context::LabelAttach{}), c->label_built.assign((size_t)RING * c->B * 2, 0);
        std::fill(c->label_built.begin(), c->label_built.end(), (uint8_t)0);
        for (int r = 0; r < RING; r++) c->label_ring[(size_t)r * c->B + seq] = Context::LabelAttach{};  // (an attachment made under the old record has the old size)
        if (!c->h_lab_stage.empty() && c->h_lab_stage[(size_t)seq]) {  // (the host calls' ring is sized by the record: reserved again by the next host call)
            (void)hipHostFree(c->h_lab_stage[(size_t)seq]);
            c->dfree(c->d_lab_ring[(size_t)seq]);
            c->h_lab_stage[(size_t)seq] = c->d_lab_ring[(size_t)seq] = nullptr;
        }
        if (cfg) give_planes(c, c->d_lmask, 2, seq, c->sensor == 2 ? 1 : 2, 64);
        c->n_label = put_seq_value(c, c->label, 1, lvt_amd_label_mask{}, seq, {cfg ? *cfg : lvt_amd_label_mask{}}, [](const lvt_amd_label_mask &r) { return r.label_width > 0; });
        return 0;
    });
}
// The label images of sequence seq's NEXT frame.  left / right: tightly packed host images (device == false) or planes in HBM at any address and the given
// pitch; NULL: that eye gets no labels; both NULL: a pending attachment is cleared.  Accepted with frames in flight: nothing here waits for them, except that a
// host call makes room the way upload_async does -- this slot's staging was read last by the copy of the frame RING places before, which has been collected then.
static int frame_labels(lvt_handle h, int seq, bool device, const void *left, int pitch_l, const void *right, int pitch_r) {
    const char *who = device ? "lvt_amd_frame_labels_device" : "lvt_amd_frame_labels";
    return with_auto_handle(h, [&](lvt_handle t) -> int {
        Context *c = frame_context(t, who, 0, true, {"a pooled handle (its frames ride a chain shared with other handles) (nothing was attached)", nullptr, nullptr});
        if (!c) return -1;
        DeviceGuard guard(c);
        try {
            if (seq < 0 || seq >= c->B) return refuse(t, who, "no sequence " + std::to_string(seq) + " in this handle (nothing was attached)");
            if (!c->has_label(seq)) return refuse(t, who, "a sequence without a label-mask record: set one with lvt_amd_set_label_mask first (nothing was attached)");
            const lvt_amd_label_mask &r = c->label[(size_t)seq];
            const void *src[2] = {left, right};
            const int pitch[2] = {device ? pitch_l : r.label_width, device ? pitch_r : r.label_width};
            for (int e = 0; e < 2; e++)
                if (src[e] && pitch[e] < r.label_width)
                    return refuse(t, who, "a label pitch of " + std::to_string(pitch[e]) + " bytes on label images " + std::to_string(r.label_width) + " pixels wide (pitch >= label_width) (nothing was attached)");
            if (right && c->sensor == 2) return refuse(t, who, "right-eye labels on an RGB-D handle (it has one image: pass NULL for the right eye) (nothing was attached)");
            if (c->early_pending) drain(c);  // (a synchronous call's frame whose pose has been returned: its tail has long finished)
            const int held = c->pend.valid ? 1 : 0;  // (the held frame owns number enq + 1 and slot enq % RING)
            const int slot = (int)((c->enq + held) % RING);
            Context::LabelAttach &A = c->label_ring[(size_t)slot * c->B + seq];
            A = Context::LabelAttach{};
            if (!left && !right) return 0;
            if (!device) {
                while (c->enq + held - c->done >= RING - 1) collect_oldest(c);
                const size_t img = (size_t)r.label_width * r.label_height, stride = (img + 15) & ~(size_t)15;
                if (c->h_lab_stage.empty()) c->h_lab_stage.assign((size_t)c->B, nullptr), c->d_lab_ring.assign((size_t)c->B, nullptr);
                if (!c->h_lab_stage[(size_t)seq]) {
                    HIPCHK(c, hipHostMalloc((void **)&c->h_lab_stage[(size_t)seq], stride * 2 * RING, hipHostMallocDefault));
                    c->d_lab_ring[(size_t)seq] = c->dalloc<uint8_t>(stride * 2 * RING);
                }
                for (int e = 0; e < 2; e++) {
                    if (!src[e]) continue;
                    const size_t off = ((size_t)slot * 2 + e) * stride;
                    std::memcpy(c->h_lab_stage[(size_t)seq] + off, src[e], img);
                    HIPCHK(c, hipMemcpyAsync(c->d_lab_ring[(size_t)seq] + off, c->h_lab_stage[(size_t)seq] + off, img, hipMemcpyHostToDevice, c->stream_f));
                    src[e] = c->d_lab_ring[(size_t)seq] + off;
                }
            }
            for (int e = 0; e < 2; e++) A.src[e] = static_cast<const uint8_t *>(src[e]), A.pitch[e] = pitch[e];
            A.frame = (long long)c->enq + held + 1;  // (written last: a refusal above leaves nothing attached)
            return 0;
        } catch (...) {
        }
        return -1;
    });
}

// ---- pose uncertainty (k_poseinfo.hip): a property of the handle like the pixel format, refused where that is refused ----------------------------------
static int enable_pose_info(lvt_handle h, int enable) {
    static const PropertyCall call = {"lvt_amd_enable_pose_info", 0, {"a pooled handle (its frames ride a chain shared with other handles) (nothing was changed)", nullptr, nullptr}, nullptr};
    return set_property(h, call, 0, true, [&](lvt_handle t, Context *c) -> int {
        if (frames_in_flight(c)) return refuse_unchanged(t, call.who, "frames in flight: enable before the first frame or after every frame has been collected");
        if ((enable != 0) == c->pose_info) return 0;
        if (enable && !c->h_pinfo) {
            HIPCHK(c, hipHostMalloc((void **)&c->h_pinfo, sizeof(lvt_amd_pose_info) * c->B * RING, hipHostMallocCoherent));
            HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_pinfo_dev, c->h_pinfo, 0));
        }
        for (int s = 0; s < c->B; s++) pose_info_clear(c, s);  // (either way: the last frame has no record)
        c->pose_info = enable != 0;
        return 0;
    });
}

// ---- what the properties' getters and the two filters' stage entries share -----------------------------------------------------------------------------
// a property's record of sequence seq: 1 with *out (may be NULL) where it has one, 0 where it has none (a seat never has one), -1: no such handle or sequence
template <typename T>
static int get_seq_record(lvt_handle h, int seq, bool (Context::*has)(int) const, std::vector<T> Context::*vec, T *out) {
    h = resolve_handle(h, false);
    if (is_slot(h)) return seq == 0 ? 0 : -1;
    if (!is_ctx(h)) return -1;
    const Context *c = static_cast<const Context *>(h);
    if (seq < 0 || seq >= c->B) return -1;
    if (!(c->*has)(seq)) return 0;
    if (out) *out = (c->*vec)[(size_t)seq];
    return 1;
}
// a filter's stats getter: out[0 .. width) zeroed, then 1 with pick(c, fc) on the FeatCtl of the frame lvt_amd_get_counts answers for, 0 where there is nothing
// to report -- a seat, no frame yet, a sequence the filter is not set for (has), a step the filter did not run in under the present records (ring is per
// STEP) or one this sequence sat out: it went through no launch in it, its FeatCtl holds an older frame's words --, -1 otherwise
template <typename Has, typename Pick>
static int get_filter_stats(lvt_handle h, int seq, int *out, int width, Has has, bool (Context::*ring)[RING], Pick pick) {
    h = resolve_handle(h);
    if (out) std::fill_n(out, width, 0);
    if (is_slot(h)) return seq == 0 ? 0 : -1;
    if (!is_ctx(h) || !out) return -1;
    Context *c = static_cast<Context *>(h);
    if (seq < 0 || seq >= c->B) return -1;
    DeviceGuard guard(c);
    try {
        drain(c);
        if (c->done == 0 || !has(c, seq) || !(c->*ring)[c->last_slot] || frame_args(c, c->last_slot, seq).absent) return 0;
        FeatCtl fc;
        d2h(c, &fc, c->h_seqs[seq].fb[c->last_par].fc, 1);
        pick(c, fc);
        return 1;
    } catch (...) {
    }
    return -1;
}
// One filter's stage entry, the part both have: the caller's n features in a host-built Seq (sequence 0, parity 0, the left eye) whose eight arrays, count and
// FeatCtl live in the call's StageScratch.  The entry fills seq().prm and featctl().in, asks upload() for the device Seq, launches, and takes fetch()'s answer.
struct StageFeatures {
    static constexpr float *Feat::*F32[6] = {&Feat::x, &Feat::y, &Feat::resp, &Feat::bx, &Feat::by, &Feat::depth};
    static constexpr int16_t *Feat::*I16[2] = {&Feat::hcx, &Feat::hcy};
    StageScratch S;
    Seq hs;
    FeatCtl fc;
    float *f[6];    // the caller's arrays, in F32's order ...
    int16_t *h[2];  // ... and in I16's
    size_t nn;
    StageFeatures(int n, float *x, float *y, float *resp, float *bx, float *by, float *depth, int16_t *hcx, int16_t *hcy) : f{x, y, resp, bx, by, depth}, h{hcx, hcy}, nn((size_t)n) {
        std::memset(&hs, 0, sizeof(hs)), std::memset(&fc, 0, sizeof(fc));
        for (int k = 0; k < 6; k++) feat().*F32[k] = S.buf<float>(nn, f[k]);
        for (int k = 0; k < 2; k++) feat().*I16[k] = S.buf<int16_t>(nn, h[k]);
        feat().n = S.buf<int>(1, &n);
    }
    Seq &seq() { return hs; }
    Feat &feat() { return hs.fb[0].feat[0]; }
    FeatCtl &featctl() { return fc; }
    // the device Seq, NULL on a HIP failure
    const Seq *upload() {
        hs.fb[0].fc = S.buf<FeatCtl>(1, &fc);
        const Seq *d = S.buf<Seq>(1, &hs);
        return S.ok() ? d : nullptr;
    }
    // behind the launch: the new count with every array back whole -- the elements behind the count hold what the kernel left there --, -1 on a HIP failure
    int fetch() {
        int n_new = -1;
        bool ok = hipGetLastError() == hipSuccess && S.fetch(&n_new, (const int *)feat().n, 1);
        for (int k = 0; k < 6; k++) ok = ok && S.fetch(f[k], (const float *)(feat().*F32[k]), nn);
        for (int k = 0; k < 2; k++) ok = ok && S.fetch(h[k], (const int16_t *)(feat().*I16[k]), nn);
        return ok ? n_new : -1;
    }
};
}  // namespace lvt

// ---- the properties' C-ABI ----------------------------------------------------------------------------------------------------------------------------
extern "C" {
LVT_API int lvt_amd_set_rectifiers(lvt_handle h, lvt_amd_rectifier left, lvt_amd_rectifier right) { return set_rectifiers(h, 0, false, left, right); }
LVT_API int lvt_amd_batch_set_rectifiers(lvt_handle h, int seq, lvt_amd_rectifier left, lvt_amd_rectifier right) { return set_rectifiers(h, seq, true, left, right); }

LVT_API int lvt_amd_set_pixel_format(lvt_handle h, int format) { return set_pixel_format(h, 0, false, format); }
LVT_API int lvt_amd_batch_set_pixel_format(lvt_handle h, int seq, int format) { return set_pixel_format(h, seq, true, format); }
LVT_API int lvt_amd_get_pixel_format(lvt_handle h, int seq) {
    h = resolve_handle(h, false);
    if (is_slot(h)) return seq == 0 ? PIX_GRAY8 : -1;
    if (!is_ctx(h)) return -1;
    const Context *c = static_cast<const Context *>(h);
    return (seq < 0 || seq >= c->B) ? -1 : c->fmt_of(seq);
}

LVT_API int lvt_amd_set_sensor_format(lvt_handle h, const lvt_amd_sensor_format *f) { return set_sensor_format(h, 0, false, f); }
LVT_API int lvt_amd_batch_set_sensor_format(lvt_handle h, int seq, const lvt_amd_sensor_format *f) { return set_sensor_format(h, seq, true, f); }
LVT_API int lvt_amd_get_sensor_format(lvt_handle h, int seq, lvt_amd_sensor_format *out) { return get_seq_record(h, seq, &Context::has_sensor, &Context::sens, out); }
LVT_API int lvt_amd_get_sensor_window(lvt_handle h, int seq, int eye, int *lo, int *hi) { return get_sensor_window(h, seq, eye, lo, hi); }
// the stage alone on caller planes: tables of one image, the null stream (an auto window: the histogram and the levels first); returns when the plane is written
LVT_API int lvt_amd_convert_sensor_device(const lvt_amd_sensor_format *f, const void *src, int src_pitch_bytes, int width, int height, uint8_t *dst, int dst_pitch,
                                          int window_out[2]) {
    const char *who = "lvt_amd_convert_sensor_device";
    if (window_out) window_out[0] = window_out[1] = 0;
    if (!f || !src || !dst) return refuse_call(who, "a NULL argument (nothing was launched)");
    if (f->format == SENSOR_NONE) return refuse_call(who, "format LVT_AMD_SENSOR_NONE converts nothing (nothing was launched)");
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return refuse_call(who, "a side outside 1 ... 16384 (nothing was launched)");
    const std::string why = sensor_format_check(*f, width, height);
    if (!why.empty()) return refuse_call(who, why + " (nothing was launched)");
    const int row = width * sensor_bpp(f->format);
    if (src_pitch_bytes < row) return refuse_call(who, "a source pitch of " + std::to_string(src_pitch_bytes) + " does not hold a row of " + std::to_string(row) + " bytes (nothing was launched)");
    if (f->format == SENSOR_MONO16 && (((uintptr_t)src | (uintptr_t)(unsigned)src_pitch_bytes) & 1))
        return refuse_call(who, "a MONO16 plane needs an even address and an even pitch (nothing was launched)");
    if (dst_pitch < width || (dst_pitch & 3) || ((uintptr_t)dst & 3))
        return refuse_call(who, "a destination pitch smaller than the width or no multiple of 4, or a destination that is not 4-byte aligned (nothing was launched)");
    const bool aut = f->format == SENSOR_MONO16 && f->auto_window != 0;
    StageScratch S;  // (lvt_stage_entries.h)
    uint32_t *hist = aut ? S.buf<uint32_t>(SENSOR_BINS) : nullptr;
    int *win = aut ? S.buf<int>(2) : nullptr;
    if (!S.ok()) return refuse_call(who, "no device memory for the histogram (nothing was launched)");
    SensorTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.im[0] = sensor_img(*f, static_cast<const uint8_t *>(src), src_pitch_bytes, width, height, dst, dst_pitch, win, hist);
    if (aut) {
        hipLaunchKernelGGL(k_sensor_hist, sensor_hist_grid((width + 1) / 2 * height, 1), dim3(SENSOR_HIST_THREADS), 0, 0, tab);
        hipLaunchKernelGGL(k_sensor_levels, dim3(1), dim3(256), 0, 0, tab);
    }
    hipLaunchKernelGGL(k_sensor_frames, dim3((unsigned)((dst_pitch / 4 * height + 255) / 256), 1), dim3(256), 0, 0, tab);
    hipError_t err = hipGetLastError();  // (the launches'; reading it clears it, so it is kept)
    if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
    if (err != hipSuccess) return refuse_call(who, hipGetErrorString(err));
    if (f->format == SENSOR_MONO16 && window_out) {
        window_out[0] = f->lo, window_out[1] = f->hi;
        if (aut && !S.fetch(window_out, win, 2)) return refuse_call(who, "the window could not be read back");
    }
    return 0;
}

LVT_API int lvt_amd_set_depth_camera(lvt_handle h, const lvt_amd_depth_camera *cam) { return set_depth_camera(h, 0, false, cam); }
LVT_API int lvt_amd_batch_set_depth_camera(lvt_handle h, int seq, const lvt_amd_depth_camera *cam) { return set_depth_camera(h, seq, true, cam); }
LVT_API int lvt_amd_get_depth_camera(lvt_handle h, int seq, lvt_amd_depth_camera *out) { return get_seq_record(h, seq, &Context::has_depth_cam, &Context::depth_cam, out); }
// the stage alone on caller data: clear, then scatter, on the caller's stream
LVT_API int lvt_amd_register_depth_device(const lvt_amd_depth_camera *cam, const lvt_amd_params *colour, const void *d_depth, int depth_pitch_bytes,
                                          int depth_format, float depth_scale, void *d_out, int out_pitch_bytes, void *hip_stream) {
    if (!cam || !colour || !d_depth || !d_out || !depth_camera_check(*cam).empty()) return -1;
    if (depth_format != DEPTH_F32 && depth_format != DEPTH_U16) return -1;
    if (depth_format == DEPTH_U16 && !(std::isfinite(depth_scale) && depth_scale > 0.f)) return -1;
    const int esz = (depth_format == DEPTH_U16) ? 2 : 4;
    if (((uintptr_t)d_depth % esz) || depth_pitch_bytes <= 0 || (depth_pitch_bytes % esz) || (long long)depth_pitch_bytes < (long long)cam->width * esz) return -1;
    if (colour->img_width < 1 || colour->img_width > 8192 || colour->img_height < 1 || colour->img_height > 8192) return -1;
    if (((uintptr_t)d_out & 3) || (out_pitch_bytes & 3) || (long long)out_pitch_bytes < (long long)colour->img_width * 4) return -1;
    DepthRegTable tab;
    std::memset(&tab, 0, sizeof(tab));
    const DepthRegImg &I = tab.im[0] = depth_reg_img(*cam, *colour, d_depth, depth_pitch_bytes / esz, depth_format, depth_scale, static_cast<float *>(d_out), out_pitch_bytes / 4);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const size_t words = (size_t)I.dst_pitch * I.H;
    if ((words + 3) / 4 / 256 + 1 > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(k_depth_clear, dim3((unsigned)(((words + 3) / 4 + 255) / 256), 1), dim3(256), 0, st, tab);
    hipLaunchKernelGGL(k_depth_register, dim3((unsigned)((I.dw * I.dh + 255) / 256), 1), dim3(256), 0, st, tab);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

LVT_API int lvt_amd_set_equalisation(lvt_handle h, const lvt_amd_equalisation *cfg) { return set_equalisation(h, 0, false, cfg); }
LVT_API int lvt_amd_batch_set_equalisation(lvt_handle h, int seq, const lvt_amd_equalisation *cfg) { return set_equalisation(h, seq, true, cfg); }
LVT_API int lvt_amd_get_equalisation(lvt_handle h, int seq, lvt_amd_equalisation *out) { return get_seq_record(h, seq, &Context::has_equal, &Context::equal, out); }
// host only: steps 1 and 2 of the definition
LVT_API int lvt_amd_equalisation_plan(const lvt_amd_equalisation *cfg, int w, int h, int out[6], float *lut_scale) {
    if (!cfg || !out || w < 1 || w > 8192 || h < 1 || h > 8192 || !equalisation_check(*cfg, w, h).empty()) return -1;
    const EqualPlan p = equalisation_plan(*cfg, w, h);
    out[0] = p.Wp, out[1] = p.Hp, out[2] = p.tile_w, out[3] = p.tile_h, out[4] = p.area, out[5] = p.clip;
    if (lut_scale) *lut_scale = p.lut_scale;
    return 0;
}
// the stage alone on caller planes: both launches on the caller's stream; the table buffer lives until the stream has run them
LVT_API int lvt_amd_equalise_device(const lvt_amd_equalisation *cfg, const void *d_src, int src_pitch, int w, int h, void *d_dst, int dst_pitch, void *hip_stream) {
    if (!cfg || !d_src || !d_dst || w < 1 || w > 8192 || h < 1 || h > 8192 || !equalisation_check(*cfg, w, h).empty()) return -1;
    if (src_pitch < w || dst_pitch < w || (dst_pitch & 3) || ((uintptr_t)d_dst & 3) || (long long)dst_pitch * h > 0x7FFFFFFFll) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StageScratch S;  // (lvt_stage_entries.h)
    uint8_t *lut = S.buf<uint8_t>((size_t)cfg->tiles_x * cfg->tiles_y * 256);
    if (!S.ok()) return -1;
    ClaheTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.im[0] = clahe_img(*cfg, static_cast<const uint8_t *>(d_src), src_pitch, w, h, static_cast<uint8_t *>(d_dst), dst_pitch, lut, clahe_direct());
    hipLaunchKernelGGL(k_clahe_lut, dim3(cfg->tiles_x * cfg->tiles_y, 1), dim3(256), 0, st, tab);
    hipLaunchKernelGGL(k_clahe_apply, dim3((unsigned)(((size_t)(dst_pitch / 4) * h + 255) / 256), 1), dim3(256), 0, st, tab);
    return hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess ? 0 : -1;
}

LVT_API int lvt_amd_set_reduction(lvt_handle h, const lvt_amd_reduction *r) { return set_reduction(h, 0, false, r); }
LVT_API int lvt_amd_batch_set_reduction(lvt_handle h, int seq, const lvt_amd_reduction *r) { return set_reduction(h, seq, true, r); }
LVT_API int lvt_amd_get_reduction(lvt_handle h, int seq, lvt_amd_reduction *out) { return get_seq_record(h, seq, &Context::has_reduce, &Context::red, out); }
// the stage alone on caller planes: a table of one image, the null stream; returns when the plane is written
LVT_API int lvt_amd_reduce_device(const void *d_src, int src_w, int src_h, int src_pitch, int factor, void *d_dst, int dst_pitch, int *launches) {
    const char *who = "lvt_amd_reduce_device";
    if (launches) *launches = 0;
    if (!d_src || !d_dst) return refuse_call(who, "a NULL argument (nothing was launched)");
    if (factor < 2 || factor > REDUCE_MAX_FACTOR) return refuse_call(who, "factor = " + std::to_string(factor) + " (2 ... 8) (nothing was launched)");
    if (src_w < factor || src_w > REDUCE_MAX_SIDE || src_h < factor || src_h > REDUCE_MAX_SIDE)
        return refuse_call(who, "a source side outside factor ... 16384 (nothing was launched)");
    const int w = src_w / factor, h = src_h / factor;
    if (src_pitch < src_w) return refuse_call(who, "a source pitch smaller than the source width (nothing was launched)");
    if (dst_pitch < w || (dst_pitch & 3) || ((uintptr_t)d_dst & 3))
        return refuse_call(who, "a destination pitch smaller than the reduced width or no multiple of 4, or a destination that is not 4-byte aligned (nothing was launched)");
    ReduceTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.im[0] = reduce_img(static_cast<const uint8_t *>(d_src), src_pitch, factor, static_cast<uint8_t *>(d_dst), dst_pitch, w, h);
    hipLaunchKernelGGL(k_reduce_frames, reduce_grid(dst_pitch / 4 * h, 1), dim3(REDUCE_THREADS), 0, 0, tab);
    if (launches) *launches = 1;
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return refuse_call(who, hipGetErrorString(hipGetLastError()));
    return 0;
}
// host only: the lens of the image k_reduce_frames writes from an image of lens *in.  Reduced pixel x covers source [f x, f x + f): f' = f / factor,
// c' = (c + 0.5) / factor - 0.5, in double; the sizes by integer division; the model and the distortion coefficients (functions of the normalised ray) unchanged
LVT_API int lvt_amd_lens_reduced(const lvt_amd_lens *in, int factor, lvt_amd_lens *out) {
    if (!in || !out || factor < 1 || factor > REDUCE_MAX_FACTOR || in->width / factor < 1 || in->height / factor < 1) return -1;
    lvt_amd_lens r = *in;
    const double f = (double)factor;
    r.width = in->width / factor, r.height = in->height / factor;
    r.K[0] = in->K[0] / f, r.K[4] = in->K[4] / f;
    r.K[2] = (in->K[2] + 0.5) / f - 0.5, r.K[5] = (in->K[5] + 0.5) / f - 0.5;
    *out = r;
    return 0;
}

LVT_API void lvt_amd_depth_guard_default(lvt_amd_depth_guard *out) {
    if (out) *out = lvt_amd_depth_guard{1, 4, 0.01f, 0.02f};
}
LVT_API int lvt_amd_set_depth_guard(lvt_handle h, const lvt_amd_depth_guard *cfg) { return set_depth_guard(h, 0, false, cfg); }
LVT_API int lvt_amd_batch_set_depth_guard(lvt_handle h, int seq, const lvt_amd_depth_guard *cfg) { return set_depth_guard(h, seq, true, cfg); }
LVT_API int lvt_amd_get_depth_guard(lvt_handle h, int seq, lvt_amd_depth_guard *out) { return get_seq_record(h, seq, &Context::has_guard, &Context::depth_guard, out); }
// out: {kept, dropped} of the frame lvt_amd_get_counts answers for; 0 for a sequence of a batch that sat the last collected step out
LVT_API int lvt_amd_get_depth_guard_stats(lvt_handle h, int seq, int out[2]) {
    return get_filter_stats(h, seq, out, 2, [](const Context *c, int s) { return c->has_guard(s); }, &Context::ring_guarded,
                            [&](const Context *, const FeatCtl &fc) { out[0] = fc.guard_kept, out[1] = fc.guard_dropped; });
}
// the stage alone on caller data (host pointers): the n features' eight arrays are compacted IN PLACE under the rule of "DEPTH GUARD" against a width x height
// depth plane of `pitch_elems` elements per row, and every array comes back whole -- the elements behind the new count hold what the kernel left there.
// Returns the new count, -1 on a refusal (lvt_amd_last_error(NULL)) or a HIP failure.
LVT_API int lvt_amd_depth_guard_features(int n, float *x, float *y, float *resp, float *bx, float *by, float *depth_of, int16_t *hcx, int16_t *hcy, const void *depth,
                                         int depth_format, float depth_scale, int width, int height, int pitch_elems, float near_plane, float far_plane,
                                         const lvt_amd_depth_guard *cfg) {
    const char *who = "lvt_amd_depth_guard_features";
    if (n < 0 || n > NF_MAX || !depth || !cfg || width < 1 || width > 8192 || height < 1 || height > 8192 || pitch_elems < width ||
        (n > 0 && (!x || !y || !resp || !bx || !by || !depth_of || !hcx || !hcy)))
        return refuse_call(who, "a NULL argument, n outside 0 ... 4096, a size outside 1 ... 8192 or a pitch smaller than the width (nothing was changed)");
    if (depth_format != DEPTH_F32 && depth_format != DEPTH_U16) return refuse_call(who, "unknown depth format " + std::to_string(depth_format) + " (nothing was changed)");
    if (depth_format == DEPTH_U16 && !(std::isfinite(depth_scale) && depth_scale > 0.f)) return refuse_call(who, "a 16-bit plane whose depth_scale is not finite and > 0 (nothing was changed)");
    const std::string why = depth_guard_check(*cfg);
    if (!why.empty()) return refuse_call(who, why + " (nothing was changed)");
    StageFeatures T(n, x, y, resp, bx, by, depth_of, hcx, hcy);
    Params &q = T.seq().prm;
    q.W = width, q.H = height, q.sensor = 2, q.near_plane = near_plane, q.far_plane = far_plane;
    FrameIn &in = T.featctl().in;
    in.depth_img = reinterpret_cast<const float *>(T.S.buf<uint8_t>((size_t)pitch_elems * height * (depth_format == DEPTH_U16 ? 2 : 4), static_cast<const uint8_t *>(depth)));
    in.depth_pitch = pitch_elems, in.depth_format = depth_format, in.depth_scale = depth_format == DEPTH_U16 ? depth_scale : 0.f;
    GuardTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.s[0] = GuardSeq{cfg->radius, cfg->min_support, cfg->tol_abs, cfg->tol_rel};
    const Seq *d_seq = T.upload();
    if (!d_seq) return refuse_call(who, hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(k_depth_guard, dim3(1, 1, 1), dim3(1024), 0, 0, d_seq, tab, 0, 0);
    const int n_new = T.fetch();
    return n_new >= 0 ? n_new : refuse_call(who, hipGetErrorString(hipGetLastError()));
}

LVT_API int lvt_amd_set_mask(lvt_handle h, const void *left, const void *right) { return set_mask(h, 0, false, false, left, 0, right, 0); }
LVT_API int lvt_amd_batch_set_mask(lvt_handle h, int seq, const void *left, const void *right) { return set_mask(h, seq, true, false, left, 0, right, 0); }
LVT_API int lvt_amd_set_mask_device(lvt_handle h, const void *d_left, int pitch_left, const void *d_right, int pitch_right) {
    return set_mask(h, 0, false, true, d_left, pitch_left, d_right, pitch_right);
}
LVT_API int lvt_amd_batch_set_mask_device(lvt_handle h, int seq, const void *d_left, int pitch_left, const void *d_right, int pitch_right) {
    return set_mask(h, seq, true, true, d_left, pitch_left, d_right, pitch_right);
}
// out: {kept left, dropped left, kept right, dropped right} of the frame lvt_amd_get_counts answers for; an eye without a mask reports 0, 0; 0 for a sequence
// of a batch that sat the last collected step out
LVT_API int lvt_amd_get_mask_stats(lvt_handle h, int seq, int out[4]) {
    // (an eye is reported where it has a static mask or the last collected step built a label plane for it: asked behind the drain, so last_slot is that step's)
    auto filtered = [](const Context *c, int s, int e) { return c->has_mask(s, e) || c->built_label(c->last_slot, s, e); };
    return get_filter_stats(h, seq, out, 4, [&](const Context *c, int s) { return filtered(c, s, 0) || filtered(c, s, 1); }, &Context::ring_masked,
                            [&](const Context *c, const FeatCtl &fc) {
                                for (int e = 0; e < 2; e++)
                                    if (filtered(c, seq, e)) out[2 * e] = fc.mask_kept[e], out[2 * e + 1] = fc.mask_dropped[e];
                            });
}
LVT_API int lvt_amd_set_label_mask(lvt_handle h, const lvt_amd_label_mask *cfg) { return set_label_mask(h, 0, false, cfg); }
LVT_API int lvt_amd_batch_set_label_mask(lvt_handle h, int seq, const lvt_amd_label_mask *cfg) { return set_label_mask(h, seq, true, cfg); }
LVT_API int lvt_amd_get_label_mask(lvt_handle h, int seq, lvt_amd_label_mask *out) { return get_seq_record(h, seq, &Context::has_label, &Context::label, out); }
LVT_API int lvt_amd_frame_labels(lvt_handle h, int seq, const void *left, const void *right) { return frame_labels(h, seq, false, left, 0, right, 0); }
LVT_API int lvt_amd_frame_labels_device(lvt_handle h, int seq, const void *d_left, int pitch_left, const void *d_right, int pitch_right) {
    return frame_labels(h, seq, true, d_left, pitch_left, d_right, pitch_right);
}
// the stage alone on caller data (host pointers): k_label_mask builds the W x H plane of "LABEL MASKS" from a label image of cfg's size and, where given, a
// static mask, into `out`, whose H rows of out_pitch bytes come back whole.  The device copies of the label image and the static mask keep the caller's
// addresses modulo 4 (an odd address stays odd), and the device plane stands between guard bytes the call checks behind the launch.  0, or -1 on a refusal
// (lvt_amd_last_error(NULL)) or a HIP failure.
LVT_API int lvt_amd_build_label_mask(const lvt_amd_label_mask *cfg, const uint8_t *labels, int label_pitch, int W, int H, const uint8_t *static_or_NULL,
                                     int static_pitch, uint8_t *out, int out_pitch) {
    const char *who = "lvt_amd_build_label_mask";
    if (!cfg || !labels || !out || W < 1 || W > 8192 || H < 1 || H > 8192 || out_pitch < W || (out_pitch & 3) || (static_or_NULL && static_pitch < W))
        return refuse_call(who, "a NULL argument, a size outside 1 ... 8192, a pitch smaller than the width or an output pitch that is no multiple of 4 (nothing was changed)");
    const std::string why = label_mask_check(*cfg);
    if (!why.empty()) return refuse_call(who, why + " (nothing was changed)");
    if (label_pitch < cfg->label_width) return refuse_call(who, "a label pitch smaller than label_width (nothing was changed)");
    constexpr size_t GUARD = 64;
    constexpr int GUARD_BYTE = 0x5A;
    StageScratch S;
    const size_t lab_bytes = (size_t)label_pitch * cfg->label_height, stat_bytes = static_or_NULL ? (size_t)static_pitch * H : 0, out_bytes = (size_t)out_pitch * H;
    const size_t lab_off = (uintptr_t)labels & 3, stat_off = (uintptr_t)static_or_NULL & 3;
    uint8_t *d_lab = S.buf<uint8_t>(lab_bytes + 4), *d_stat = static_or_NULL ? S.buf<uint8_t>(stat_bytes + 4) : nullptr;
    uint8_t *d_out = S.buf<uint8_t>(out_bytes + 2 * GUARD, nullptr, GUARD_BYTE);
    if (!S.ok() || hipMemcpy(d_lab + lab_off, labels, lab_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        (d_stat && hipMemcpy(d_stat + stat_off, static_or_NULL, stat_bytes, hipMemcpyHostToDevice) != hipSuccess))
        return refuse_call(who, hipGetErrorString(hipGetLastError()));
    LabelTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.im[0] = label_img(*cfg, d_lab + lab_off, label_pitch, W, H, d_stat ? d_stat + stat_off : nullptr, static_pitch, d_out + GUARD, out_pitch);
    hipLaunchKernelGGL(k_label_mask, dim3(label_tiles(out_pitch, H), 1), dim3(256), 0, 0, tab);
    std::vector<uint8_t> back(out_bytes + 2 * GUARD);
    if (hipGetLastError() != hipSuccess || !S.fetch(back.data(), (const uint8_t *)d_out, back.size())) return refuse_call(who, hipGetErrorString(hipGetLastError()));
    for (size_t k = 0; k < GUARD; k++)
        if (back[k] != GUARD_BYTE || back[GUARD + out_bytes + k] != GUARD_BYTE) return refuse_call(who, "the kernel wrote outside the plane");
    std::memcpy(out, back.data() + GUARD, out_bytes);
    return 0;
}
// the stage alone on caller data (host pointers): the n features' eight arrays are compacted IN PLACE under the rule of "FEATURE MASKS" against a width x height
// mask of `pitch` bytes per row, and every array comes back whole -- the elements behind the new count hold what the kernel left there.  Returns the new
// count, -1 on a refusal (lvt_amd_last_error(NULL)) or a HIP failure.
LVT_API int lvt_amd_mask_features(int n, float *x, float *y, float *resp, float *bx, float *by, float *depth, int16_t *hcx, int16_t *hcy, const uint8_t *mask,
                                  int width, int height, int pitch) {
    const char *who = "lvt_amd_mask_features";
    if (n < 0 || n > NF_MAX || !mask || width < 1 || width > 8192 || height < 1 || height > 8192 || pitch < width ||
        (n > 0 && (!x || !y || !resp || !bx || !by || !depth || !hcx || !hcy)))
        return refuse_call(who, "a NULL argument, n outside 0 ... 4096, a size outside 1 ... 8192 or a pitch smaller than the width (nothing was changed)");
    StageFeatures T(n, x, y, resp, bx, by, depth, hcx, hcy);
    Params &q = T.seq().prm;
    q.W = width, q.H = height, q.sensor = 1;
    MaskTable tab;
    std::memset(&tab, 0, sizeof(tab));
    tab.s[0].mask[0] = T.S.buf<uint8_t>((size_t)pitch * height, mask), tab.s[0].pitch[0] = pitch;
    const Seq *d_seq = T.upload();
    if (!d_seq) return refuse_call(who, hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(k_mask_features, dim3(1, 1, 1), dim3(1024), 0, 0, d_seq, tab, 0, 0);
    const int n_new = T.fetch();
    return n_new >= 0 ? n_new : refuse_call(who, hipGetErrorString(hipGetLastError()));
}

LVT_API int lvt_amd_enable_pose_info(lvt_handle h, int enable) { return enable_pose_info(h, enable); }
LVT_API int lvt_amd_get_pose_info(lvt_handle h, int seq, lvt_amd_pose_info *out) {
    h = resolve_handle(h);
    if (!out) return -1;
    std::memset(out, 0, sizeof(*out));
    if (is_slot(h)) return seq == 0 ? 0 : -1;  // (a seat never has it enabled)
    if (!is_ctx(h)) return -1;
    Context *c = static_cast<Context *>(h);
    if (seq < 0 || seq >= c->B) return -1;
    if (!c->pose_info) return 0;
    DeviceGuard guard(c);
    try {
        drain(c);  // (as lvt_amd_get_pose / lvt_amd_get_counts: the last frame enqueued, collected)
        *out = c->h_pinfo[(size_t)c->last_slot * c->B + seq];
        return 1;
    } catch (...) {
    }
    return -1;
}
}  // extern "C"
