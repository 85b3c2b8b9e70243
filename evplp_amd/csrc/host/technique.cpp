// The host side of the reference's technique plugin, restated above the C ABI:
//   main()                      reflectcuts/main.cpp:87-121      -> evplp_render_json
//   RtTechnique::render         rt/rttechnique.h:6-9             -> ComPhotonTechnique::render
//   RtComPhoton::render / run   rt/rtcomphoton/rtcomphoton.h:107-223, 883-1133
//   RtLvcComPhoton              rt/rtcomphoton/rtlvccomphoton.h  -> ComPhotonTechnique(lvc = true)
//   RtPt2::render / run         rt/rtpt/rtpt2.h:84-116, 575-719  -> PathTraceTechnique
// Same JSON keys, defaults, errors and outputs (three images + stat file); no window, no GL:
// the frame loop of common/realtime.h reduces to the iteration cap and the wall-clock limit.
#include "../../../include/evplp.h"
#include "images.hpp"
#include "json.hpp"
#include "scene_io.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

namespace evplp {

namespace {
// build-only key "bvhBuilder"
int parse_bvh_builder(const std::string &v) {
    if (v == "sah") return EVPLP_BVH_SAH;
    if (v == "sbvh") return EVPLP_BVH_SBVH;
    if (v == "lbvh") return EVPLP_BVH_LBVH;
    if (v == "gpu") return EVPLP_BVH_LBVH_GPU;
    if (v == "ploc") return EVPLP_BVH_PLOC_GPU;
    throw std::runtime_error("bvhBuilder: expected \"sah\", \"sbvh\", \"lbvh\", \"gpu\" or \"ploc\", got \"" + v + "\"");
}
const std::map<std::string, int> kFrameModes = { { "accumulate", 1 }, { "cleareveryframe", 2 } };   // rtcomphoton.h:1194-1197
const std::map<std::string, int> kMisModes = { { "one", 0 }, { "balance", 1 }, { "max", 2 }, { "power2", 3 },
                                               { "geometryClamp", 4 }, { "geometryBrdfClamp", 5 } }; // :1199-1206
constexpr float kInvPi = 0.318309886183790671537767526745028724068919291480912897495f;

// The techniques always run on an evplp_group (one rank = the reference's single device); the `device` block of the technique
// JSON asks for more ranks: {"gpus": N, "virtual": bool, "stripRows": R, "rccl": bool} (build-only key, include/evplp.h).
struct Grp {   // RAII for the C handle
    evplp_group *g = nullptr;
    ~Grp() { if (g) evplp_group_destroy(g); }
};
void check(evplp_group *g, int rc, const char *what) {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + evplp_group_last_error(g));
}
// What the `device` block says about the RUN (the rest of it configures the group, create_group):
//   "deal": "cost" | "roundRobin" -- row blocks dealt by the cost a calibration frame clocks (evplp_group_calibrate / _rebalance), or block b to
//           rank b % N.  Default: by cost when the run has more than one rank, a VPL / VSL gather, and enough iterations for the calibration
//           frame -- one more frame -- to pay for itself (5 from six ranks on, 25 from three, 100 at two); results do not depend on it.
//   "exchangeEvery": k -- the strips are all-gathered (every GPU holds the frame) in every k-th iteration's composite; 0 = never inside the
//           loop.  Default 0: this loop is headless -- nothing looks at the assembled frame between the frames that are WRITTEN
//           (rtcomphoton.h:1079-1102, 1124-1132), and those always exchange; 1 is what the reference's per-iteration runFinalProgram to
//           the window amounts to (:997-1004): a host barrier and an all-gather per iteration, which a sub-millisecond iteration feels
//           (profiles/r06_host_feed.txt).  Every rank still composites its strip every iteration.  Results do not depend on it.
//   "partition": "strips" | "iterations" -- what the N GPUs share out.  "strips" (default): the image, as above.  "iterations" (the photonfam
//           techniques in accumulate mode): the ITERATIONS of the progressive run -- one group of N EVPLP_PARTITION_ITERATIONS ranks, GPU g
//           renders iterations g, g + N, g + 2N, ... of the whole image (each has its own seed, jitter and radius: rtcomphoton.h:936-1063 makes
//           an iteration depend on its number only; evplp_group_select_rank before its passes), nothing is exchanged while the loop runs
//           ("exchangeEvery": k > 0 reduces in every k-th iteration), and the accumulators are summed on the GPUs -- in rank order,
//           reduce_shards_kernel -- whenever a frame is written.  Under a time limit the loop waits only for the rank the next iteration
//           reuses, so the N GPUs work at once.  N times the iterations per second with no replicated work and nothing to balance; a single
//           iteration is no faster, every GPU holds whole-image buffers, and the VPL / photon sums are associated differently from one GPU's
//           (images agree to fp32 round-off, ~1e-7, not bit for bit).  The emitter image is one GPU's exactly: the light plane is never cleared
//           in accumulate mode, so it is the union over the iterations of the pixels where the un-jittered emitter passed the depth test
//           against the jittered scene, and the reduction takes the first non-zero pixel in rank order -- the same colour wherever any rank
//           wrote it.  What config #4 wants: its iteration is two latency-bound walks that row strips cannot shorten.
struct RunOptions { int deal = -1; int exchange_every = 0; bool shard_iterations = false; };       // deal: -1 default, 0 round robin, 1 by cost
RunOptions run_options(const Json &json) {
    RunOptions o;
    if (!json.has("device")) return o;
    const Json &d = json.at("device");
    if (d.has("deal")) {
        const std::string v = d.at("deal").as_string("device.deal");
        if (v == "cost") o.deal = 1; else if (v == "roundRobin") o.deal = 0; else throw JsonError("device.deal: \"cost\" or \"roundRobin\"");
    }
    if (d.has("partition")) {
        const std::string v = d.at("partition").as_string("device.partition");
        if (v == "iterations") o.shard_iterations = true; else if (v != "strips") throw JsonError("device.partition: \"strips\" or \"iterations\"");
    }
    if (d.has("exchangeEvery")) { o.exchange_every = (int)d.at("exchangeEvery").as_int("device.exchangeEvery"); if (o.exchange_every < 0) throw JsonError("device.exchangeEvery: must be >= 0"); }
    return o;
}
// iterations: the ranks share out the iterations ("partition": "iterations", EVPLP_PARTITION_ITERATIONS) instead of row strips
void create_group(Grp &grp, const evplp_config &cfg, const Json &json, int device, bool iterations = false) {
    evplp_group_config gc; std::memset(&gc, 0, sizeof(gc));
    gc.n_ranks = 1; gc.strip_rows = 0;      // (0: the group's default, 16-row strips)
    bool virt = false;
    if (json.has("device")) {
        const Json &d = json.at("device");
        if (d.has("gpus")) gc.n_ranks = (int)d.at("gpus").as_int("device.gpus");
        if (d.has("virtual")) virt = d.at("virtual").as_bool("device.virtual");
        if (d.has("stripRows")) gc.strip_rows = (int)d.at("stripRows").as_int("device.stripRows");
        if (d.has("rccl")) gc.use_rccl = d.at("rccl").as_bool("device.rccl") ? 1 : 0;
        if (d.has("stripCapacityPct")) gc.strip_capacity_pct = (int)d.at("stripCapacityPct").as_int("device.stripCapacityPct");
        if (d.has("splitLightPaths")) gc.split_light_paths = d.at("splitLightPaths").as_bool("device.splitLightPaths") ? 1 : -1;   // (absent: the library's cost model)
    }
    if (gc.n_ranks < 1 || gc.n_ranks > 64) throw JsonError("device.gpus: must be 1..64");
    if (iterations) gc.partition = EVPLP_PARTITION_ITERATIONS;
    std::vector<int32_t> devs((size_t)gc.n_ranks);
    for (int r = 0; r < gc.n_ranks; r++) devs[(size_t)r] = virt ? device : device + r;
    gc.devices = devs.data();
    int rc = evplp_group_create(&cfg, &gc, &grp.g);
    if (rc < 0) throw std::runtime_error(std::string("evplp_group_create: ") + evplp_group_last_error(nullptr));
}
int device_gpus(const Json &json) {
    if (!json.has("device") || !json.at("device").has("gpus")) return 1;
    const int n = (int)json.at("device").at("gpus").as_int("device.gpus");
    if (n < 1 || n > 64) throw JsonError("device.gpus: must be 1..64");
    return n;
}
void upload_scene_group(evplp_group *g, const HostScene &scene) {
    for (int r = 0; r < evplp_group_size(g); r++) {
        evplp_context *h = evplp_group_context(g, r);
        if (upload_scene(h, scene) < 0) throw std::runtime_error(std::string("scene upload: ") + evplp_last_error(h));
    }
}
// setupPhotonSplatIcosohedron("sphere/icosphere.obj") (rtcomphoton.h:632-644, 677): the proxy mesh the photon splat draws around every
// photon.  The reference opens the path relative to its working directory; here it is looked for there and next to the scene JSON, and
// a build-only key "splatProxy" names another file.  The asset is a Git-LFS pointer in the reference's repository: when no mesh file
// is found (or the file is such a pointer) the generated 42-vertex / 80-face icosphere stands in (evplp_default_splat_proxy) and a
// note says so.  A file that IS a mesh but not a closed convex one is an error (evplp_set_splat_proxy refuses it).
// Build-only key "splatFootprint": "proxy" (default: the reference's coverage rule) | "ideal" (the radius test alone).
uint32_t setup_splat_footprint(evplp_group *g, const Json &json, const std::string &json_dir) {
    std::string mode = json.has("splatFootprint") ? json.at("splatFootprint").as_string("splatFootprint") : std::string("proxy");
    if (mode == "ideal") return (uint32_t)EVPLP_FOOTPRINT_IDEAL;
    if (mode != "proxy") throw JsonError("splatFootprint: expected \"proxy\" or \"ideal\", got \"" + mode + "\"");
    std::vector<std::string> candidates;
    const bool named = json.has("splatProxy");
    if (named) candidates.push_back(join_path(json_dir, json.at("splatProxy").as_string("splatProxy")));
    else { candidates.push_back("sphere/icosphere.obj"); candidates.push_back(join_path(json_dir, "sphere/icosphere.obj")); }
    for (const std::string &path : candidates) {
        { std::ifstream probe(path); if (!probe) { if (named) throw std::runtime_error("Impossible to load the scene: " + path); continue; } }
        MeshData m;
        try { m = load_single_mesh_obj(path); }
        catch (const std::exception &e) {
            if (std::string(e.what()).find("Git-LFS pointer") == std::string::npos) throw;
            std::fprintf(stderr, "note: %s is a Git-LFS pointer; the photon splat uses the generated 42-vertex icosphere as its proxy\n", path.c_str());
            break;
        }
        check(g, evplp_group_set_splat_proxy(g, m.verts.data(), (int32_t)(m.verts.size() / 3), m.idx.data(), (int32_t)(m.idx.size() / 3)), ("photon splat proxy " + path).c_str());
        return (uint32_t)EVPLP_FOOTPRINT_PROXY;
    }
    check(g, evplp_group_set_splat_proxy(g, nullptr, 0, nullptr, 0), "photon splat proxy");
    return (uint32_t)EVPLP_FOOTPRINT_PROXY;
}
// Output files named in the technique block.  The shipped scene files carry the authors' Windows paths
// ("C://result/conference/3_pm.pfm"): off Windows a drive-letter path keeps only its file name and lands next to
// the scene JSON, so those files run unchanged; every other path is used as the reference would (relative to the
// working directory there, to the JSON's directory here).
std::string output_path(const std::string &out_dir, const std::string &name) {
    if (name.size() > 1 && name[1] == ':' && ((name[0] >= 'A' && name[0] <= 'Z') || (name[0] >= 'a' && name[0] <= 'z'))) {
        size_t cut = name.find_last_of("/\\");
        std::string base = cut == std::string::npos ? name.substr(2) : name.substr(cut + 1);
        std::fprintf(stderr, "note: output \"%s\" has a drive letter; writing %s/%s\n", name.c_str(), out_dir.c_str(), base.c_str());
        return out_dir + "/" + base;
    }
    return join_path(out_dir, name);
}
// FloatImage::FlipY (floatimage.cpp:114-128) of a bottom-up RGB image + row de-interleave
std::vector<float> flip_y(const std::vector<float> &rgb, int w, int h) {
    std::vector<float> out((size_t)w * h * 3);
    for (int row = 0; row < h; row++) std::memcpy(&out[(size_t)row * w * 3], &rgb[(size_t)(h - 1 - row) * w * 3], sizeof(float) * 3 * w);
    return out;
}
// build-only additions to the stat file: per-pass device times of the last iteration
void add_pass_times(evplp_group *g, Json &st) {
    evplp_context *h = evplp_group_context(g, 0);
    const char *names[EVPLP_PASS_COUNT] = { "primaryMs", "lightTraceMs", "gatherVplMs", "gatherVslMs", "splatMs", "resolveMs", "pathTraceMs", "gatherLvcMs" };
    for (int p = 0; p < EVPLP_PASS_COUNT; p++) { evplp_pass_stats ps; if (evplp_pass_stats_get(h, p, &ps) == EVPLP_OK && ps.ms > 0) st.set(names[p], Json::number(ps.ms)); }
}
// IndependentSampler(mRngOffset).nextVec2() (common/rng.h:9-44, sampler/independent.h:37-40) as the reference's own headers
// behave when compiled here with g++ 11 / libstdc++ (pinned by tests/golden/jitter.npz, generated from oracle/_ref):
//   * std::uniform_real_distribution<float>(0, 1) over std::mt19937 = generate_canonical<float, 24>: float(x) / 2^32 with the
//     32-bit draw x converted to float by round-to-nearest, and a result of 1.0 replaced by the float below it;
//   * Vec2(nextFloat(), nextFloat()): g++ evaluates the two arguments right to left, so .y takes the FIRST draw.
// Both are implementation-defined in C++; the authors built with MSVC, whose library and argument order may differ --
// statistically equivalent, but a different jitter sequence.
struct JitterSampler {
    std::mt19937 rng;
    explicit JitterSampler(uint32_t seed) : rng(seed) {}
    float next() { float u = (float)(uint32_t)rng() / 4294967296.0f; return u >= 1.0f ? 0.99999994f : u; }
    // ndc jitter (2 u - 1) * invResolution (rtcomphoton.h:946-952, rtpt2.h:617-623)
    void next_jitter(int W, int H, float jitter[2]) {
        float uy = next(), ux = next();
        jitter[0] = (2.0f * ux - 1.0f) * (1.0f / (float)W); jitter[1] = (2.0f * uy - 1.0f) * (1.0f / (float)H);
    }
};
// a file named in the technique block that cannot be read (evplp_render_json: EVPLP_ERR_IO)
struct IoError : std::runtime_error { using std::runtime_error::runtime_error; };

// Build-only key "convergence" (not a reference key; the reference leaves error curves to external scripts): the error of the image the
// run saves as its result against a reference image, measured on the device at checkpoints of the running loop (evplp_group_frame_error:
// 32 bytes per image row come to the host, nothing else) and written as one JSON file.
//   {"reference": "ref.pfm", "mask": "mask.png", "everyIterations": 10, "everyMs": 250, "stopRelMse": 0.01, "filename": "curve.json"}
// reference (PFM / HDR, evplp_load_image) and filename are required; mask (evplp_decode_image) is optional; paths resolve as splatProxy's.
// Checkpoints: after iteration i (counted from 1) when everyIterations divides i; when the wall clock has passed the next multiple of
// everyMs (missed multiples are skipped); always one after the loop's last synchronise, unless the last one already saw that iteration.  A
// checkpoint waits as the loop does before it looks at the clock, takes timeMs (wall clock since the loop's start, earlier checkpoints'
// overhead included) and then measures; the time inside the error call is summed as overheadMs.  A time limit stays wall clock, overhead
// included.  stopRelMse ends the run at the first checkpoint whose relMSE (the masked one with a mask) is <= it.  Everything is validated
// before the group exists: a bad block costs no GPU time.
class Convergence {
public:
    bool on = false;
    void parse(const Json &tech, const std::string &json_dir, const std::string &out_dir, int W, int H) {
        if (!tech.has("convergence")) return;
        const Json &c = tech.at("convergence");
        if (!c.is_object()) throw JsonError("convergence: expected an object");
        for (const char *k : { "reference", "filename" }) if (!c.has(k)) throw JsonError(std::string("convergence.") + k + ": missing required key");
        reference = c.at("reference").as_string("convergence.reference");
        filename = output_path(out_dir, c.at("filename").as_string("convergence.filename"));
        if (c.has("everyIterations")) {
            every_iterations = c.at("everyIterations").as_int("convergence.everyIterations");
            if (every_iterations <= 0) throw JsonError("convergence.everyIterations: must be > 0");
        }
        if (c.has("everyMs")) {
            every_ms = c.at("everyMs").as_number("convergence.everyMs");
            if (!(every_ms > 0.0)) throw JsonError("convergence.everyMs: must be > 0");
            next_ms = every_ms;
        }
        if (c.has("stopRelMse")) {
            stop_rel_mse = c.at("stopRelMse").as_number("convergence.stopRelMse");
            if (!(stop_rel_mse >= 0.0)) throw JsonError("convergence.stopRelMse: must be >= 0");
        }
        const std::string ref_path = join_path(json_dir, reference);
        int32_t w = 0, h = 0;
        if (evplp_load_image(ref_path.c_str(), &w, &h, nullptr, 0) != EVPLP_OK) throw IoError("convergence.reference: cannot read " + ref_path);
        if (w != W || h != H)
            throw JsonError("convergence.reference: " + ref_path + " is " + std::to_string(w) + " x " + std::to_string(h) + ", the scene renders " + std::to_string(W) + " x " + std::to_string(H));
        ref.resize((size_t)W * H * 3);
        if (evplp_load_image(ref_path.c_str(), &w, &h, ref.data(), ref.size()) != EVPLP_OK) throw IoError("convergence.reference: cannot read " + ref_path);
        if (c.has("mask")) {
            const std::string mask_path = join_path(json_dir, c.at("mask").as_string("convergence.mask"));
            int32_t ch = 0;
            if (evplp_decode_image(mask_path.c_str(), &w, &h, &ch, nullptr, 0) != EVPLP_OK) throw IoError("convergence.mask: cannot read " + mask_path);
            if (w != W || h != H)
                throw JsonError("convergence.mask: " + mask_path + " is " + std::to_string(w) + " x " + std::to_string(h) + ", the scene renders " + std::to_string(W) + " x " + std::to_string(H));
            mask.resize((size_t)W * H * 3);
            if (evplp_decode_image(mask_path.c_str(), &w, &h, &ch, mask.data(), mask.size()) != EVPLP_OK) throw IoError("convergence.mask: cannot read " + mask_path);
            for (size_t i = 0; i < (size_t)W * H; i++) kept += (mask[3 * i] | mask[3 * i + 1] | mask[3 * i + 2]) != 0 ? 1 : 0;
        }
        pixels = (int64_t)W * H;
        on = true;
    }
    void upload(evplp_group *g) const {
        if (on) check(g, evplp_group_set_error_reference(g, ref.data(), mask.empty() ? nullptr : mask.data()), "convergence reference");
    }
    // "animation": this frame's file (name: Animation::frame_path)
    template <class Name> void name_files(Name name) { filename = name(filename); }
    // after iteration i of the loop, the host clock at hand (no wait yet)
    bool due(int i, double now_ms) const {
        return on && ((every_iterations > 0 && i % every_iterations == 0) || (every_ms > 0.0 && now_ms >= next_ms));
    }
    // wait_and_clock: the loop's wait, then the wall clock.  Returns true when stopRelMse is reached.
    template <class WaitAndClock>
    bool checkpoint(evplp_group *g, int i, WaitAndClock wait_and_clock, float vs, float ps, float ls, int32_t mask_emitter) {
        const double t = wait_and_clock();
        const auto t0 = std::chrono::steady_clock::now();
        Point p; p.iteration = i; p.time_ms = t;
        check(g, evplp_group_frame_error(g, vs, ps, ls, mask_emitter, 0, p.e), "convergence");
        overhead_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        points.push_back(p);
        if (every_ms > 0.0) next_ms = (std::floor(t / every_ms) + 1.0) * every_ms;
        return stop_rel_mse >= 0.0 && (mask.empty() ? p.e[1] : p.e[2]) <= stop_rel_mse;
    }
    // the final checkpoint (after the loop's last synchronise): none when the last one saw this iteration already
    void finish(evplp_group *g, int i, double now_ms, float vs, float ps, float ls, int32_t mask_emitter) {
        if (!on) return;
        if (points.empty() || points.back().iteration != i) checkpoint(g, i, [&] { return now_ms; }, vs, ps, ls, mask_emitter);
        std::string s = "{\n    \"reference\": " + quoted(reference) + ",\n    \"pixels\": " + std::to_string(pixels) + ",\n";
        if (!mask.empty()) s += "    \"keptPixels\": " + std::to_string(kept) + ",\n";
        s += "    \"overheadMs\": " + num(overhead_ms) + ",\n    \"checkpoints\": [";
        for (size_t k = 0; k < points.size(); k++) {
            const Point &p = points[k];
            s += std::string(k ? ",\n" : "\n") + "        {\"iteration\": " + std::to_string(p.iteration) + ", \"timeMs\": " + num(p.time_ms) +
                 ", \"mse\": " + num(p.e[0]) + ", \"relMse\": " + num(p.e[1]);
            if (!mask.empty()) s += ", \"relMseMasked\": " + num(p.e[2]);
            s += "}";
        }
        s += "\n    ]\n}\n";
        std::ofstream of(filename);
        if (!of || !(of << s)) throw std::runtime_error("cannot write " + filename);
    }

private:
    struct Point { int iteration = 0; double time_ms = 0.0; double e[3] = { 0.0, 0.0, 0.0 }; };
    static std::string num(double v) { if (!std::isfinite(v)) return "null"; char b[40]; std::snprintf(b, sizeof b, "%.17g", v); return b; }     // (every bit of the double)
    static std::string quoted(const std::string &v) { Json j = Json::string(v); return j.dump(); }
    std::string reference, filename;
    std::vector<float> ref; std::vector<uint8_t> mask;
    int64_t pixels = 0, kept = 0;
    long long every_iterations = 0;
    double every_ms = 0.0, next_ms = 0.0, stop_rel_mse = -1.0, overhead_ms = 0.0;
    std::vector<Point> points;
};

// Build-only key "noise" (not a reference key): the error of the image the run saves, estimated from the spread between its own iterations
// -- no reference image -- on the device (evplp_group_noise_*: 32 bytes per image row come to the host) and written as one JSON file.
//   {"batchIterations": 1, "everyIterations": 10, "everyMs": 250, "stopRelMse": 0.01, "mask": "m.png", "filename": "noise.json",
//    "varianceFilename": "var.pfm"}
// filename is required.  Every batchIterations iterations of a shard (the whole group on row strips; each rank of an iteration partition, of
// its own iterations) close one batch (evplp_group_noise_fold).  Checkpoints fall at a fold: when everyIterations (a multiple of
// batchIterations) divides the iteration count, or at the first fold after the wall clock has passed the next multiple of everyMs; they need
// two folds, and time themselves as "convergence" does.  After the loop every shard folds the iterations it holds unfolded and one last
// checkpoint is taken.  stopRelMse ends the run at the first checkpoint whose relMSE (the masked one with a mask) is <= it.
// varianceFilename: the per-pixel variance of the saved combined image, rows top to bottom.  frameMode "cleareveryframe" keeps no running
// sum to fold: refused.  Everything is validated before the group exists.
class Noise {
public:
    bool on = false;
    // the "adaptive" block's tile counts (Adaptive below): written into every checkpoint when `adaptive` is set
    bool adaptive = false; long long retired_tiles = 0, image_tiles = 0;
    // ... and, under "adaptiveSampling.budget", the samples the next call will run (the sum of the tiles' s_t): "budgetSamples"
    bool budget = false; long long budget_samples = 0;
    long long batch_iterations() const { return batch; }
    long long batch_count() const { return batches; }
    void parse(const Json &tech, const std::string &json_dir, const std::string &out_dir, int W, int H, int frame_mode) {
        if (!tech.has("noise")) return;
        const Json &c = tech.at("noise");
        if (!c.is_object()) throw JsonError("noise: expected an object");
        if (!c.has("filename")) throw JsonError("noise.filename: missing required key");
        if (frame_mode == 2) throw JsonError("noise: frameMode \"cleareveryframe\" keeps no running sum to fold");
        filename = output_path(out_dir, c.at("filename").as_string("noise.filename"));
        if (c.has("batchIterations")) {
            batch = c.at("batchIterations").as_int("noise.batchIterations");
            if (batch <= 0 || batch > INT32_MAX) throw JsonError("noise.batchIterations: must be > 0");
        }
        if (c.has("everyIterations")) {
            every_iterations = c.at("everyIterations").as_int("noise.everyIterations");
            if (every_iterations <= 0) throw JsonError("noise.everyIterations: must be > 0");
            if (every_iterations % batch != 0) throw JsonError("noise.everyIterations: must be a multiple of noise.batchIterations");
        }
        if (c.has("everyMs")) {
            every_ms = c.at("everyMs").as_number("noise.everyMs");
            if (!(every_ms > 0.0)) throw JsonError("noise.everyMs: must be > 0");
            next_ms = every_ms;
        }
        if (c.has("stopRelMse")) {
            stop_rel_mse = c.at("stopRelMse").as_number("noise.stopRelMse");
            if (!(stop_rel_mse >= 0.0)) throw JsonError("noise.stopRelMse: must be >= 0");
        }
        if (c.has("varianceFilename")) variance_filename = output_path(out_dir, c.at("varianceFilename").as_string("noise.varianceFilename"));
        if (c.has("mask")) {
            const std::string mask_path = join_path(json_dir, c.at("mask").as_string("noise.mask"));
            int32_t w = 0, h = 0, ch = 0;
            if (evplp_decode_image(mask_path.c_str(), &w, &h, &ch, nullptr, 0) != EVPLP_OK) throw IoError("noise.mask: cannot read " + mask_path);
            if (w != W || h != H)
                throw JsonError("noise.mask: " + mask_path + " is " + std::to_string(w) + " x " + std::to_string(h) + ", the scene renders " + std::to_string(W) + " x " + std::to_string(H));
            mask.resize((size_t)W * H * 3);
            if (evplp_decode_image(mask_path.c_str(), &w, &h, &ch, mask.data(), mask.size()) != EVPLP_OK) throw IoError("noise.mask: cannot read " + mask_path);
            for (size_t i = 0; i < (size_t)W * H; i++) kept += (mask[3 * i] | mask[3 * i + 1] | mask[3 * i + 2]) != 0 ? 1 : 0;
        }
        pixels = (int64_t)W * H;
        on = true;
    }
    template <class Name> void name_files(Name name) { filename = name(filename); if (!variance_filename.empty()) variance_filename = name(variance_filename); }
    // tracking starts from the sums as they are (after the loop's clear); shards: 1, or the ranks of an iteration partition
    void start(evplp_group *g, int shards) {
        if (!on) return;
        check(g, evplp_group_noise_track(g, 1, mask.empty() ? nullptr : mask.data()), "noise tracking");
        own.assign((size_t)shards, 0); folded.assign((size_t)shards, 0);
    }
    // after an iteration of `shard` (the selected rank of an iteration partition): folds when its batch is full; true when it folded
    bool after_iteration(evplp_group *g, int shard) {
        if (!on) return false;
        const size_t r = (size_t)shard;
        if (++own[r] - folded[r] < batch) return false;
        fold(g, r, batch);
        return true;
    }
    bool due(int i, double now_ms, bool folded_now) const {
        return on && folded_now && batches >= 2 && ((every_iterations > 0 && i % every_iterations == 0) || (every_ms > 0.0 && now_ms >= next_ms));
    }
    // as Convergence::checkpoint; the figure of the image scale * sums + ls * light
    template <class WaitAndClock>
    bool checkpoint(evplp_group *g, int i, WaitAndClock wait_and_clock, float scale, float ls, int32_t mask_emitter) {
        const double t = wait_and_clock();
        const auto t0 = std::chrono::steady_clock::now();
        Point p; p.iteration = i; p.time_ms = t; p.batches = batches; p.retired = retired_tiles; p.budget_samples = budget_samples;
        check(g, evplp_group_noise_estimate(g, scale, ls, mask_emitter, p.e), "noise");
        overhead_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        points.push_back(p);
        if (every_ms > 0.0) next_ms = (std::floor(t / every_ms) + 1.0) * every_ms;
        return stop_rel_mse >= 0.0 && (mask.empty() ? p.e[1] : p.e[2]) <= stop_rel_mse;
    }
    // after the loop's last synchronise: every shard's unfolded iterations as one more batch, the last checkpoint, the files
    void finish(evplp_group *g, int i, double now_ms, float scale, float ls, int32_t mask_emitter, int W, int H) {
        if (!on) return;
        bool more = false;
        for (size_t r = 0; r < own.size(); r++) {
            if (own[r] == folded[r]) continue;
            if (own.size() > 1) check(g, evplp_group_select_rank(g, (int32_t)r), "select rank");
            fold(g, r, own[r] - folded[r]);
            more = true;
        }
        if (batches >= 2 && (more || points.empty() || points.back().iteration != i)) checkpoint(g, i, [&] { return now_ms; }, scale, ls, mask_emitter);
        std::string s = "{\n    \"pixels\": " + std::to_string(pixels) + ",\n";
        if (!mask.empty()) s += "    \"keptPixels\": " + std::to_string(kept) + ",\n";
        s += "    \"batchIterations\": " + std::to_string(batch) + ",\n    \"overheadMs\": " + num(overhead_ms) + ",\n    \"checkpoints\": [";
        for (size_t k = 0; k < points.size(); k++) {
            const Point &p = points[k];
            s += std::string(k ? ",\n" : "\n") + "        {\"iteration\": " + std::to_string(p.iteration) + ", \"timeMs\": " + num(p.time_ms) +
                 ", \"batches\": " + std::to_string(p.batches) + ", \"mse\": " + num(p.e[0]) + ", \"relMse\": " + num(p.e[1]);
            if (!mask.empty()) s += ", \"relMseMasked\": " + num(p.e[2]);
            if (adaptive) s += ", \"retiredTiles\": " + std::to_string(p.retired) + ", \"activeTiles\": " + std::to_string(image_tiles - p.retired);
            if (budget) s += ", \"budgetSamples\": " + std::to_string(p.budget_samples);
            s += "}";
        }
        s += "\n    ]\n}\n";
        std::ofstream of(filename);
        if (!of || !(of << s)) throw std::runtime_error("cannot write " + filename);
        if (variance_filename.empty()) return;
        if (batches < 2) { std::printf("note: noise: %lld fold(s), no variance image (%s) without two\n", batches, variance_filename.c_str()); return; }
        std::vector<float> var((size_t)W * H * 3);
        check(g, evplp_group_noise_variance(g, scale, var.data()), "noise variance");
        std::vector<float> top = flip_y(var, W, H);
        if (save_image(variance_filename.c_str(), W, H, top.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + variance_filename);
    }

private:
    struct Point { int iteration = 0; double time_ms = 0.0; long long batches = 0; double e[3] = { 0.0, 0.0, 0.0 }; long long retired = 0, budget_samples = 0; };
    static std::string num(double v) { if (!std::isfinite(v)) return "null"; char b[40]; std::snprintf(b, sizeof b, "%.17g", v); return b; }     // (every bit of the double)
    void fold(evplp_group *g, size_t r, long long k) {
        check(g, evplp_group_noise_fold(g, (int32_t)k), "noise fold");
        folded[r] += k; batches++;
    }
    std::string filename, variance_filename;
    std::vector<uint8_t> mask;
    int64_t pixels = 0, kept = 0;
    long long batch = 1, every_iterations = 0, batches = 0;
    double every_ms = 0.0, next_ms = 0.0, stop_rel_mse = -1.0, overhead_ms = 0.0;
    std::vector<long long> own, folded;      // per shard: iterations run, iterations folded
    std::vector<Point> points;
};

// A run whose outputs are written but whose request cannot be met (evplp_render_json returns EVPLP_ERR_INVALID)
struct InvalidError : std::runtime_error { using std::runtime_error::runtime_error; };

// Build-only key "denoise" (photonfam, lvcphotonfam, pt): the saved composite filtered by the variance-guided a-trous denoiser
// (evplp_group_denoise) and written as one more image, rows top to bottom, in the format of the file's extension.
//   {"filename": "denoised.pfm", "levels": 5, "sigmaLuminance": 4, "sigmaNormal": 128, "sigmaPosition": 0.01}
// filename is required; the others default to the library's (include/evplp.h).  Needs the "noise" block, whose variance guides the filter
// (so frameMode "cleareveryframe" is refused).  Validated before the group exists.  Written after every other output, behind the noise
// block's last fold; with fewer than two folds the other outputs are written and the run fails with EVPLP_ERR_INVALID.
//   "temporal": {"maxHistory": 16, "normalCos": 0.9}   (both optional; only with an "animation" block)
// accumulates over the frames of the animation in front of the filter (evplp_group_denoise_temporal): every frame's file comes from that
// call, frame 0's is the file of the run without the key, and a frame's stat file gains "temporalReprojected", "temporalDisoccluded" and
// "temporalMeanHistory".  The accumulation takes the frames for independent samples: set "animation": {"rngAdvance": k} with
// k >= numMaxIteration, or every frame repeats the same noise pattern and nothing is gained.  Refused without an "animation" block (a single
// frame has no history), with an unknown key inside and with values out of range (maxHistory 1 .. 1024, normalCos in (0, 1]).
class Denoise {
public:
    bool on = false;
    // (before Noise::parse: a "cleareveryframe" run with both blocks is refused under this block's name)
    void parse(const Json &tech, const std::string &out_dir, int frame_mode) {
        if (!tech.has("denoise")) return;
        const Json &c = tech.at("denoise");
        if (!c.is_object()) throw JsonError("denoise: expected an object");
        if (!c.has("filename")) throw JsonError("denoise.filename: missing required key");
        filename = output_path(out_dir, c.at("filename").as_string("denoise.filename"));
        if (frame_mode == 2) throw JsonError("denoise: frameMode \"cleareveryframe\" keeps no running sum for the noise block to fold");
        if (!tech.has("noise")) throw JsonError("denoise: needs a \"noise\" block (its per-pixel variance guides the filter)");
        if (c.has("levels")) {
            const long long l = c.at("levels").as_int("denoise.levels");
            if (l < 1 || l > 10) throw JsonError("denoise.levels: must be 1..10");
            p.levels = (int32_t)l;
        }
        sigma(c, "sigmaLuminance", p.sigma_luminance);
        sigma(c, "sigmaNormal", p.sigma_normal);
        sigma(c, "sigmaPosition", p.sigma_position);
        if (c.has("temporal")) {
            const Json &t = c.at("temporal");
            if (!t.is_object()) throw JsonError("denoise.temporal: expected an object");
            if (!tech.has("animation")) throw JsonError("denoise.temporal: needs an \"animation\" block (a single frame has no history to accumulate)");
            for (const auto &kv : t.obj)
                if (kv.first != "maxHistory" && kv.first != "normalCos") throw JsonError("denoise.temporal." + kv.first + ": unknown key (maxHistory, normalCos)");
            if (t.has("maxHistory")) {
                const double m = t.at("maxHistory").as_number("denoise.temporal.maxHistory");
                if (!(m >= 1.0) || !(m <= 1024.0) || m != std::floor(m)) throw JsonError("denoise.temporal.maxHistory: must be an integer 1 .. 1024");
                tp.max_history = (int32_t)m;
            }
            if (t.has("normalCos")) {
                const double v = t.at("normalCos").as_number("denoise.temporal.normalCos");
                if (!std::isfinite(v) || !(v > 0.0) || v > 1.0) throw JsonError("denoise.temporal.normalCos: must be in (0, 1]");
                tp.normal_cos = (float)v;
            }
            temporal = true;
        }
        on = true;
    }
    template <class Name> void name_files(Name name) { filename = name(filename); }
    // "temporal": enabled on the group once, before the first frame
    void start(evplp_group *g) { if (on && temporal) check(g, evplp_group_temporal_enable(g, 1), "denoise.temporal"); }
    // "temporal": the frame's image, in front of its stat file (which reports the call's counts); write() saves it
    void accumulate(evplp_group *g, int W, int H, long long batches, float scale, float ls, int32_t mask_emitter) {
        if (!on || !temporal || batches < 2) return;
        held.assign((size_t)W * H * 3, 0.f);
        check(g, evplp_group_denoise_temporal(g, scale, ls, mask_emitter, &p, &tp, held.data(), &info), "denoise.temporal");
    }
    void add_stat(Json &st) const {
        if (held.empty()) return;
        st.set("temporalReprojected", Json::number((double)info.reprojected));
        st.set("temporalDisoccluded", Json::number((double)info.disoccluded));
        st.set("temporalMeanHistory", Json::number(info.filtered > 0 ? (double)info.history_sum / (double)info.filtered : 0.0));
    }
    void write(evplp_group *g, int W, int H, long long batches, float scale, float ls, int32_t mask_emitter) {
        if (!on) return;
        if (batches < 2)
            throw InvalidError("denoise: " + std::to_string(batches) + " noise batch(es) closed, the filter needs >= 2: " + filename + " is not written");
        std::vector<float> rgb((size_t)W * H * 3);
        if (!held.empty()) rgb = held;
        else check(g, evplp_group_denoise(g, scale, ls, mask_emitter, &p, rgb.data()), "denoise");
        std::vector<float> top = flip_y(rgb, W, H);
        if (save_image(filename.c_str(), W, H, top.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + filename);
    }

private:
    static void sigma(const Json &c, const char *key, float &out) {
        if (!c.has(key)) return;
        const double v = c.at(key).as_number((std::string("denoise.") + key).c_str());
        if (!std::isfinite(v) || !(v > 0.0)) throw JsonError(std::string("denoise.") + key + ": must be > 0");
        out = (float)v;
    }
    std::string filename;
    evplp_denoise_params p{};
    bool temporal = false; evplp_temporal_params tp{}; evplp_temporal_info info{}; std::vector<float> held;
};

// Build-only key "adaptive" (photonfam, VPL and VSL gathers): tiles whose estimated noise has converged stop receiving gather work
// (evplp_group_adaptive_*).  {"tileRelMse": 0.002, "everyIterations": 10, "minBatches": 4, "iterationsFilename": "iters.pfm"}
// tileRelMse is required (>= 0); everyIterations (default: noise.batchIterations) is a multiple of noise.batchIterations: at every fold whose
// iteration count it divides, the group retires -- with the loop's own 1 / i scale -- the tiles whose mean relative variance is <= tileRelMse
// once the tracker has >= minBatches (default 2, >= 2) folds.  Needs the "noise" block, whose checkpoints then carry "retiredTiles" /
// "activeTiles"; refused for lvcphotonfam and pt, under "partition": "iterations" and with frameMode "cleareveryframe".  iterationsFilename:
// every pixel's n_t / N (1 where its tile never retired), rows top to bottom.  Everything is validated before the group exists.
// pt takes the same block under the key "adaptiveSampling" (the path tracer retires the tiles; its loop ends once none is active).
// There it may hold "budget": {"minSamples": 1, "referenceQuantile": 1.0} (the defaults; needs "samplesPerCall" > 1): no tile retires; at
// every everyIterations fold the loop reads the tiles' noise with its own 1 / i scale and their sample counts, plans with S = samplesPerCall
// (evplp_plan_budgets) and sets the tiles' budgets for the calls that follow.  tileRelMse 0 then means "never stop a tile"; the loop ends
// when every budget is 0.  The checkpoints gain "budgetSamples"; "activeTiles" counts the tiles whose budget is not 0.
// photonfam's "adaptive" takes "budget" too: {"window": 16, "minSamples": 1, "referenceQuantile": 1.0} -- gather budget mode
// (evplp_group_adaptive_enable(g, 2)): a tile takes the first b_t of every `window` gathers; everyIterations is a multiple of window, the plan
// uses S = window, the loop ends when every budget is 0.  Refused where the loop would splat photons (the mode has no place for them).
class Adaptive {
public:
    // key: "adaptive" (photonfam: the gathers retire tiles) or "adaptiveSampling" (pt: the path tracer does, evplp_group_adaptive_enable_pt)
    explicit Adaptive(const char *block_key = "adaptive", bool path_trace = false) : key(block_key), pt(path_trace) {}
    bool on = false;
    // pt: no tile is active any more -- the loop has nothing left to sample
    bool all_retired(const Noise &noise) const { return on && noise.image_tiles > 0 && noise.retired_tiles >= noise.image_tiles; }
    // gathers only: every budget is 0 -- the loop has nothing left to gather (retirement alone never ends photonfam's loop: photons go on)
    bool budget_spent(const Noise &noise) const { return budget && all_retired(noise); }
    void parse(const Json &tech, const std::string &out_dir, int frame_mode, bool lvc, bool iterations_partition, Noise &noise, bool splats_photons = false) {
        if (!tech.has(key)) return;
        const Json &c = tech.at(key);
        if (!c.is_object()) throw JsonError(key + ": expected an object");
        if (lvc) throw JsonError(key + ": not for lvcphotonfam (VPL and VSL gathers only)");
        if (!noise.on) throw JsonError(key + ": needs a \"noise\" block (retirement uses its estimate)");
        if (frame_mode == 2) throw JsonError(key + ": frameMode \"cleareveryframe\" keeps no running sum");
        if (iterations_partition) throw JsonError(key + ": not under \"partition\": \"iterations\" (the ranks' decisions are not pooled)");
        if (!c.has("tileRelMse")) throw JsonError(key + ".tileRelMse: missing required key");
        tau = c.at("tileRelMse").as_number((key + ".tileRelMse").c_str());
        if (!(tau >= 0.0)) throw JsonError(key + ".tileRelMse: must be >= 0");
        every = noise.batch_iterations();
        if (c.has("everyIterations")) {
            every = c.at("everyIterations").as_int((key + ".everyIterations").c_str());
            if (every <= 0) throw JsonError(key + ".everyIterations: must be > 0");
            if (every % noise.batch_iterations() != 0) throw JsonError(key + ".everyIterations: must be a multiple of noise.batchIterations");
        }
        if (c.has("minBatches")) {
            const long long mb = c.at("minBatches").as_int((key + ".minBatches").c_str());
            if (mb < 2 || mb > INT32_MAX) throw JsonError(key + ".minBatches: must be >= 2");
            min_batches = (int32_t)mb;
        }
        if (c.has("iterationsFilename")) iterations_filename = output_path(out_dir, c.at("iterationsFilename").as_string((key + ".iterationsFilename").c_str()));
        if (c.has("budget")) {
            const Json &b = c.at("budget");
            if (!b.is_object()) throw JsonError(key + ".budget: expected an object");
            if (!pt && splats_photons) throw JsonError(key + ".budget: not with the photon splat (run.photonSplat and a photon radius > 0): a tile's VPL part would have n_t samples and its photon part N");
            if (b.has("minSamples")) budget_min = b.at("minSamples").as_int((key + ".budget.minSamples").c_str());
            if (b.has("referenceQuantile")) budget_q = b.at("referenceQuantile").as_number((key + ".budget.referenceQuantile").c_str());
            if (!(budget_q > 0.0) || !(budget_q <= 1.0)) throw JsonError(key + ".budget.referenceQuantile: must be in (0, 1]");
            if (!pt) {      // the gathers: the window takes samplesPerCall's place
                long long window = 16;
                if (b.has("window")) window = b.at("window").as_int((key + ".budget.window").c_str());
                if (window < 1 || window > 64) throw JsonError(key + ".budget.window: must be 1 .. 64");
                if (every % window != 0) throw JsonError(key + ".everyIterations: must be a multiple of " + key + ".budget.window");
                if (budget_min < 1 || budget_min > window) throw JsonError(key + ".budget.minSamples: must be 1 .. window");
                budget_samples_per_call = (int32_t)window;
            } else if (b.has("window")) throw JsonError(key + ".budget.window: the gathers' key (pt's window is samplesPerCall)");
            budget = noise.budget = true;
        }
        noise.adaptive = true;
        on = true;
    }
    template <class Name> void name_files(Name name) { if (!iterations_filename.empty()) iterations_filename = name(iterations_filename); }
    // once "samplesPerCall" is known (pt parses it behind this block)
    void parse_budget_samples(int samples_per_call) {
        if (!budget || !pt) return;
        if (samples_per_call <= 1) throw JsonError(key + ".budget: needs \"samplesPerCall\" > 1 (a budget is a share of a batched call)");
        if (budget_min < 1 || budget_min > samples_per_call) throw JsonError(key + ".budget.minSamples: must be 1 .. samplesPerCall");
        budget_samples_per_call = samples_per_call;
    }
    // before the loop's first gather (after the clear and any rebalance: N = 0)
    void start(evplp_group *g, int W, int H, Noise &noise) {
        if (!on) return;
        check(g, pt ? evplp_group_adaptive_enable_pt(g, budget ? 2 : 1) : evplp_group_adaptive_enable(g, budget ? 2 : 1), key.c_str());
        if (budget && !pt) check(g, evplp_group_adaptive_budget_window(g, budget_samples_per_call), (key + ".budget.window").c_str());
        noise.image_tiles = (long long)((W + 7) / 8) * ((H + 7) / 8);
        if (budget) {
            noise.budget_samples = noise.image_tiles * budget_samples_per_call;
            tile_rel.assign((size_t)noise.image_tiles, 0.0); tile_n.assign((size_t)noise.image_tiles, 0); tile_budget.assign((size_t)noise.image_tiles, 0);
        }
    }
    // after the fold of iteration i (folded_now): the retirement, when due
    void after_fold(evplp_group *g, int i, bool folded_now, float scale, Noise &noise) {
        if (!on || !folded_now || i % every != 0) return;
        if (budget) {
            if (noise.batch_count() < min_batches) return;
            const int32_t nt = (int32_t)tile_n.size();
            check(g, evplp_group_adaptive_tile_noise(g, scale, 1.0f, 0, tile_rel.data(), nt), "adaptive tile noise");
            check(g, evplp_group_adaptive_tiles(g, tile_n.data(), nt), "adaptive tiles");
            if (evplp_plan_budgets(tile_rel.data(), tile_n.data(), nt, budget_samples_per_call, (int32_t)budget_min, tau, budget_q, tile_budget.data()) != EVPLP_OK)
                throw std::runtime_error(key + ".budget: the tiles' noise figures are not finite");
            check(g, evplp_group_adaptive_set_budgets(g, tile_budget.data(), nt), "adaptive budgets");
            noise.retired_tiles = 0; noise.budget_samples = 0;
            for (int32_t b : tile_budget) { noise.retired_tiles += b == 0 ? 1 : 0; noise.budget_samples += b; }
            return;
        }
        const int rc = evplp_group_adaptive_retire(g, scale, 1.0f, 0, tau, min_batches);
        check(g, rc, "adaptive retire");
        noise.retired_tiles += rc;
    }
    void finish(evplp_group *g, int n, int W, int H) {
        if (!on || iterations_filename.empty()) return;
        const int tx = (W + 7) / 8, ty = (H + 7) / 8;
        std::vector<int32_t> tiles((size_t)tx * ty);
        check(g, evplp_group_adaptive_tiles(g, tiles.data(), (int32_t)tiles.size()), "adaptive tiles");
        std::vector<float> rgb((size_t)W * H * 3);
        for (int y = 0; y < H; y++)                  // (y = 0 at the bottom, as the tile map's rows)
            for (int x = 0; x < W; x++) {
                const float v = n > 0 ? (float)((double)tiles[(size_t)(y / 8) * tx + x / 8] / (double)n) : 1.0f;
                for (int ch = 0; ch < 3; ch++) rgb[((size_t)y * W + x) * 3 + ch] = v;
            }
        std::vector<float> top = flip_y(rgb, W, H);
        if (save_image(iterations_filename.c_str(), W, H, top.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + iterations_filename);
    }

private:
    std::string key; bool pt;
    double tau = 0.0;
    long long every = 1;
    int32_t min_batches = 2;
    std::string iterations_filename;
    bool budget = false; long long budget_min = 1; double budget_q = 1.0; int32_t budget_samples_per_call = 0;
    std::vector<double> tile_rel; std::vector<int32_t> tile_n, tile_budget;
};

// Build-only key "animation" (photonfam, lvcphotonfam, pt; not a reference key): the scene moves between F frames, by one row-major 3 x 4
// matrix per track and frame (evplp_group_transform_mesh: the rest pose under the matrix, nothing composes), and every frame is rendered by
// the technique's loop from its beginning.
//   {"frames": F, "tracks": [{"object": k, "matrices": [[12 numbers], ... F of them]}, {"mesh": i, "matrices": [...]}],
//    "refitPolicy": {"maxCostRatio": r, "rebuildBuilder": "gpu"}, "rotations": k, "rngAdvance": k}
// "rngAdvance": k >= 0 (default 0): frame f runs with rngOffset + f k, seeds and jitter stream both, so that its files are those of a fresh
// evplp_render_json of the moved scene with that rngOffset; with 0 every frame uses the same seeds.
// "rotations": k = 0 .. 8 (default 0: off) is evplp_group_set_refit_rotations: k passes of tree rotations inside every frame's refit.
// A track may carry, in place of "matrices", "skin" and "poses" (below, parse_poses): its mesh is then posed by bones, one palette per frame.
// A "mesh" track may also carry "morph" and "weights" (below, parse_morph) -- alone, beside "matrices", or beside "skin" + "poses": its mesh
// is then morphed by one weight set per frame, and the matrix or the pose acts on the morphed base (per frame: weights, then matrix or pose,
// then the refit).
// "object": k addresses every mesh the k-th entry of the scene file's "scene" array produced (an OBJ yields one mesh per material group),
// "object": "arealight" the light, "mesh": i the i-th mesh in upload order.  For frame f = 0 .. F - 1 every track's f-th matrix is applied,
// the tree is refitted (evplp_group_refit_accel; refitPolicy is evplp_group_set_refit_policy) and the loop runs as a fresh evplp_render_json
// of the moved scene would: accumulators, noise moments, adaptive records, iteration counter, radius schedule, jitter stream and seeds start
// again.  Every file the block writes gets _fNNNN in front of its extension; a frame's stat file gains "frame", "refitMs" (the refit's device
// time, while pass profiling is on), "refitLastAction" and, under a policy, "refitCostRatio" (cost / built_cost).  A frame's length must not
// depend on the clock: a timeLimitMs that can end the loop (< 1e8) is refused and numMaxIteration must be > 0.  Validated before the group exists.
class Animation {
public:
    bool on = false;
    int frames = 1;
    void parse(const Json &tech, const HostScene &scene, float time_limit_ms, int num_max_iteration) {
        if (!tech.has("animation")) return;
        const Json &a = tech.at("animation");
        if (!a.is_object()) throw JsonError("animation: expected an object");
        if (!a.has("frames")) throw JsonError("animation.frames: missing required key");
        const long long F = a.at("frames").as_int("animation.frames");
        if (F < 1 || F > 9999) throw JsonError("animation.frames: must be 1 .. 9999");
        if (time_limit_ms < 1e8f) throw JsonError("animation: not with a timeLimitMs that can end the loop (< 1e8): a frame's length must not depend on the clock");
        if (num_max_iteration <= 0) throw JsonError("animation: numMaxIteration must be > 0 (it alone ends a frame)");
        if (!a.has("tracks") || !a.at("tracks").is_array()) throw JsonError("animation.tracks: expected an array");
        const Json &ts = a.at("tracks");
        std::vector<char> taken(scene.meshes.size(), 0);
        for (size_t t = 0; t < ts.size(); t++) {
            const std::string where = "animation.tracks[" + std::to_string(t) + "]";
            const Json &tr = ts.at(t);
            if (!tr.is_object()) throw JsonError(where + ": expected an object");
            if (tr.has("object") == tr.has("mesh")) throw JsonError(where + ": exactly one of \"object\" and \"mesh\"");
            Track track;
            if (tr.has("mesh")) {
                const long long i = tr.at("mesh").as_int((where + ".mesh").c_str());
                if (i < 0 || i >= (long long)scene.meshes.size()) throw JsonError(where + ".mesh: " + std::to_string(i) + " is out of range (" + std::to_string(scene.meshes.size()) + " meshes)");
                track.meshes.push_back((int32_t)i);
            } else if (tr.at("object").type == Json::String) {
                if (tr.at("object").str != "arealight") throw JsonError(where + ".object: an index into \"scene\", or \"arealight\"");
                track.meshes.push_back(scene.light_mesh);
            } else {
                const long long k = tr.at("object").as_int((where + ".object").c_str());
                const long long n = (long long)scene.object_first.size() - 1;
                if (k < 0 || k >= n) throw JsonError(where + ".object: " + std::to_string(k) + " is out of range (\"scene\" has " + std::to_string(std::max(n, 0LL)) + " entries)");
                for (int32_t m = scene.object_first[(size_t)k]; m < scene.object_first[(size_t)k + 1]; m++) track.meshes.push_back(m);
            }
            for (int32_t m : track.meshes) {
                if (taken[(size_t)m]) throw JsonError(where + ": mesh " + std::to_string(m) + " is in two of the animation.tracks");
                taken[(size_t)m] = 1;
            }
            if (tr.has("morph") || tr.has("weights")) {
                parse_morph(tr, where, (size_t)F, scene, track);
                if (!tr.has("matrices") && !tr.has("poses") && !tr.has("skin")) {     // (morphed alone)
                    tracks.push_back(std::move(track));
                    continue;
                }
            }
            if (tr.has("matrices") && tr.has("poses")) throw JsonError(where + ".poses: not beside \"matrices\" (a track has exactly one of the two)");
            if (tr.has("poses")) {
                parse_poses(tr, where, (size_t)F, track);
                tracks.push_back(std::move(track));
                continue;
            }
            if (tr.has("skin")) throw JsonError(where + ".skin: only with \"poses\"");
            const std::string mw = where + ".matrices";
            if (!tr.has("matrices") || !tr.at("matrices").is_array() || (long long)tr.at("matrices").size() != F)
                throw JsonError(mw + ": expected animation.frames (" + std::to_string(F) + ") matrices of 12 numbers (or, in its place, \"skin\" and \"poses\")");
            for (size_t f = 0; f < (size_t)F; f++) {
                const Json &m = tr.at("matrices").at(f);
                if (!m.is_array() || m.size() != 12) throw JsonError(mw + "[" + std::to_string(f) + "]: expected 12 numbers (a row-major 3 x 4 matrix)");
                for (size_t k = 0; k < 12; k++) {
                    const float v = m.at(k).as_float((mw + "[" + std::to_string(f) + "]").c_str());
                    if (!std::isfinite(v)) throw JsonError(mw + "[" + std::to_string(f) + "]: entry " + std::to_string(k) + " is not a finite fp32 number");
                    track.matrices.push_back(v);
                }
            }
            tracks.push_back(std::move(track));
        }
        if (a.has("refitPolicy")) {
            const Json &p = a.at("refitPolicy");
            if (!p.is_object() || !p.has("maxCostRatio")) throw JsonError("animation.refitPolicy.maxCostRatio: missing required key");
            policy_ratio = p.at("maxCostRatio").as_number("animation.refitPolicy.maxCostRatio");
            if (!std::isfinite(policy_ratio) || !(policy_ratio >= 0.0)) throw JsonError("animation.refitPolicy.maxCostRatio: must be finite and >= 0");
            if (p.has("rebuildBuilder")) {
                try { policy_builder = parse_bvh_builder(p.at("rebuildBuilder").as_string("animation.refitPolicy.rebuildBuilder")); }
                catch (const JsonError &) { throw; }
                catch (const std::exception &e) { throw JsonError(std::string("animation.refitPolicy.rebuildBuilder: ") + e.what()); }
                // (evplp_set_refit_policy refuses PLOC as a rebuild builder for now, include/evplp.h; said here, before the group exists)
                if (policy_builder == EVPLP_BVH_PLOC_GPU)
                    throw JsonError("animation.refitPolicy.rebuildBuilder: \"ploc\" is not a rebuild builder yet (evplp_set_refit_policy); with \"bvhBuilder\": \"ploc\" leave it out -- the policy then rebuilds with the context's own builder");
            }
        }
        if (a.has("rotations")) {           // tree rotations inside every frame's refit (evplp_group_set_refit_rotations); 0, the default: off
            const double k = a.at("rotations").as_number("animation.rotations");
            if (a.at("rotations").type != Json::Number || !(k >= 0.0) || !(k <= 8.0) || k != std::floor(k)) throw JsonError("animation.rotations: must be an integer 0 .. 8 (rotation passes inside a frame's refit; 0: off)");
            rotations = (int)k;
        }
        if (a.has("rngAdvance")) {
            const double k = a.at("rngAdvance").as_number("animation.rngAdvance");
            if (a.at("rngAdvance").type != Json::Number || !(k >= 0.0) || !(k <= 1.0e6) || k != std::floor(k)) throw JsonError("animation.rngAdvance: must be an integer 0 .. 1000000 (frame f runs with rngOffset + f * rngAdvance)");
            rng_advance = (uint32_t)k;
        }
        frames = (int)F; on = true;
    }
    // frame f's rngOffset
    uint32_t frame_rng_offset(uint32_t rng_offset, int f) const { return rng_offset + (uint32_t)f * rng_advance; }
    // path with _fNNNN in front of its extension
    std::string frame_path(const std::string &path) const {
        if (!on) return path;
        char tag[16]; std::snprintf(tag, sizeof tag, "_f%04d", frame);
        const size_t slash = path.find_last_of("/\\"), dot = path.find_last_of('.');
        if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return path + tag;
        return path.substr(0, dot) + tag + path.substr(dot);
    }
    void start(evplp_group *g) {
        // (the skins of the "poses" tracks, once: what evplp_set_mesh_skin refuses about the loaded scene -- the vertex count -- is refused here)
        for (size_t t = 0; on && t < tracks.size(); t++) if (tracks[t].targets > 0)
            check(g, evplp_group_set_mesh_morph(g, tracks[t].meshes[0], tracks[t].targets, tracks[t].deltas.data(), (int32_t)(tracks[t].deltas.size() / (3 * (size_t)tracks[t].targets))),
                  ("animation.tracks[" + std::to_string(t) + "].morph").c_str());
        for (size_t t = 0; on && t < tracks.size(); t++) if (tracks[t].bones > 0)
            check(g, evplp_group_set_mesh_skin(g, tracks[t].meshes[0], tracks[t].bones, tracks[t].indices.data(), tracks[t].weights.data(), (int32_t)(tracks[t].indices.size() / 4)),
                  ("animation.tracks[" + std::to_string(t) + "].skin").c_str());
        if (on && policy_ratio > 0.0) check(g, evplp_group_set_refit_policy(g, policy_ratio, policy_builder), "animation.refitPolicy");
        if (on && rotations > 0) check(g, evplp_group_set_refit_rotations(g, rotations), "animation.rotations");
    }
    // frame f: the tracks' matrices, the refit, and its figures for the frame's stat file
    void begin_frame(evplp_group *g, int f) {
        if (!on) return;
        frame = f;
        for (const Track &t : tracks) {
            if (t.targets > 0) check(g, evplp_group_morph_mesh(g, t.meshes[0], &t.morph_weights[(size_t)t.targets * (size_t)f], t.targets), "animation: morph");
            if (t.matrices.empty()) continue;       // (morphed alone)
            if (t.bones > 0) { check(g, evplp_group_pose_mesh(g, t.meshes[0], &t.matrices[12 * (size_t)t.bones * (size_t)f], t.bones), "animation: pose"); continue; }
            for (int32_t m : t.meshes) check(g, evplp_group_transform_mesh(g, m, &t.matrices[12 * (size_t)f]), "animation: transform");
        }
        check(g, evplp_group_refit_accel(g), "animation: refit");
        refit_ms = 0.f; last_action = 0; cost_ratio = 0.0;
        evplp_context *h0 = evplp_group_context(g, 0);
        if (evplp_refit_info(h0, nullptr, nullptr, &refit_ms) < 0) throw std::runtime_error(std::string("animation: refit info: ") + evplp_last_error(h0));
        if (policy_ratio > 0.0) {
            struct evplp_accel_quality q;
            check(g, evplp_group_accel_quality(g, &q), "animation: tree cost");
            last_action = q.last_action; cost_ratio = q.built_cost > 0.0 ? q.cost / q.built_cost : 0.0;
        }
    }
    void add_stat(Json &st) const {
        if (!on) return;
        st.set("frame", Json::number(frame));
        if (refit_ms > 0.f) st.set("refitMs", Json::number(refit_ms));
        st.set("refitLastAction", Json::number(last_action));
        if (policy_ratio > 0.0) st.set("refitCostRatio", Json::number(cost_ratio));
    }

private:
    // matrices: [frames][12]; a "poses" track (bones > 0): [frames][bones][12], and the skin of its one mesh, [vertices][4] each
    // a track with "morph" (targets > 0): deltas [targets][vertices][3] and morph_weights [frames][targets], with or without matrices
    struct Track { std::vector<int32_t> meshes; std::vector<float> matrices; int32_t bones = 0; std::vector<int32_t> indices; std::vector<float> weights;
                   int32_t targets = 0; std::vector<float> deltas, morph_weights; };
    // {"mesh": i, "morph": {"targets": [[[dx, dy, dz] x vertices] x T]}, "weights": [[T numbers] x F]}: frame f morphs the mesh by its f-th
    // weight set (evplp_group_morph_mesh: the rest pose + the weighted deltas, nothing composes); the targets are set once
    // (evplp_group_set_mesh_morph).  Vertex v is the loader's numbering, so only "mesh" can carry targets.
    static void parse_morph(const Json &tr, const std::string &where, size_t F, const HostScene &scene, Track &track) {
        const std::string mw = where + ".morph", ww = where + ".weights", tw = mw + ".targets";
        if (!tr.has("morph")) throw JsonError(mw + ": \"weights\" needs morph targets ({\"targets\"})");
        if (tr.has("object")) throw JsonError(mw + ": not with \"object\" (one entry of \"scene\" yields several meshes: per-vertex data needs \"mesh\")");
        if (!tr.has("weights")) throw JsonError(ww + ": \"morph\" needs one weight set per frame");
        if (!tr.at("morph").is_object() || !tr.at("morph").has("targets") || !tr.at("morph").at("targets").is_array()) throw JsonError(tw + ": expected a list of targets, each a list of one [dx, dy, dz] per vertex");
        const Json &tg = tr.at("morph").at("targets");
        const size_t T = tg.size(), nv = scene.meshes[(size_t)track.meshes[0]].verts.size() / 3;
        if (T < 1 || T > 64) throw JsonError(tw + ": must hold 1 .. 64 targets, not " + std::to_string(T));
        for (size_t k = 0; k < T; k++) {
            const std::string kw = tw + "[" + std::to_string(k) + "]";
            if (!tg.at(k).is_array() || tg.at(k).size() != nv) throw JsonError(kw + ": expected one [dx, dy, dz] per vertex of mesh " + std::to_string(track.meshes[0]) + " (" + std::to_string(nv) + " vertices)");
            for (size_t v = 0; v < nv; v++) {
                const Json &d = tg.at(k).at(v);
                const std::string vw = kw + "[" + std::to_string(v) + "]";
                if (!d.is_array() || d.size() != 3) throw JsonError(vw + ": expected three numbers");
                for (size_t r = 0; r < 3; r++) {
                    const float x = d.at(r).as_float(vw.c_str());
                    if (!std::isfinite(x)) throw JsonError(vw + ": entry " + std::to_string(r) + " is not a finite fp32 number");
                    track.deltas.push_back(x);
                }
            }
        }
        if (!tr.at("weights").is_array() || tr.at("weights").size() != F) throw JsonError(ww + ": expected animation.frames (" + std::to_string(F) + ") weight sets of " + std::to_string(T) + " numbers");
        for (size_t f = 0; f < F; f++) {
            const Json &w = tr.at("weights").at(f);
            const std::string fw = ww + "[" + std::to_string(f) + "]";
            if (!w.is_array() || w.size() != T) throw JsonError(fw + ": expected " + std::to_string(T) + " numbers (one per target)");
            for (size_t k = 0; k < T; k++) {
                const float x = w.at(k).as_float(fw.c_str());
                if (!std::isfinite(x)) throw JsonError(fw + ": entry " + std::to_string(k) + " is not a finite fp32 number");
                track.morph_weights.push_back(x);
            }
        }
        track.targets = (int32_t)T;
    }
    // {"mesh": i, "skin": {"bones": B, "indices": [[b0, b1, b2, b3], ... one per vertex], "weights": [[w0, w1, w2, w3], ...]},
    //  "poses": [[[12 numbers] x B] x F]}: frame f poses the mesh by its f-th palette (evplp_group_pose_mesh: the rest pose skinned, nothing
    // composes); the skin is set once (evplp_group_set_mesh_skin).  Vertex v is the loader's numbering (evplp_mesh_vertices returns it), so only
    // "mesh" can carry a skin: one "object" yields several meshes.
    static void parse_poses(const Json &tr, const std::string &where, size_t F, Track &track) {
        if (tr.has("object")) throw JsonError(where + ".poses: not with \"object\" (one entry of \"scene\" yields several meshes: per-vertex data needs \"mesh\")");
        if (!tr.has("skin") || !tr.at("skin").is_object()) throw JsonError(where + ".skin: \"poses\" needs a skin ({\"bones\", \"indices\", \"weights\"})");
        const Json &sk = tr.at("skin");
        if (!sk.has("bones")) throw JsonError(where + ".skin.bones: missing required key");
        const long long B = sk.at("bones").as_int((where + ".skin.bones").c_str());
        if (B < 1 || B > 1024) throw JsonError(where + ".skin.bones: must be 1 .. 1024");
        const std::string iw = where + ".skin.indices", ww = where + ".skin.weights";
        if (!sk.has("indices") || !sk.at("indices").is_array()) throw JsonError(iw + ": expected one list of four bone indices per vertex");
        if (!sk.has("weights") || !sk.at("weights").is_array()) throw JsonError(ww + ": expected one list of four weights per vertex");
        if (sk.at("indices").size() != sk.at("weights").size())
            throw JsonError(ww + ": " + std::to_string(sk.at("weights").size()) + " entries beside " + std::to_string(sk.at("indices").size()) + " of " + iw + " (one of each per vertex)");
        for (size_t v = 0; v < sk.at("indices").size(); v++) {
            const Json &bi = sk.at("indices").at(v), &wi = sk.at("weights").at(v);
            if (!bi.is_array() || bi.size() != 4) throw JsonError(iw + "[" + std::to_string(v) + "]: expected four bone indices");
            if (!wi.is_array() || wi.size() != 4) throw JsonError(ww + "[" + std::to_string(v) + "]: expected four weights");
            for (size_t k = 0; k < 4; k++) {
                const long long b = bi.at(k).as_int((iw + "[" + std::to_string(v) + "]").c_str());
                if (b < 0 || b >= B) throw JsonError(iw + "[" + std::to_string(v) + "]: bone " + std::to_string(b) + " is outside [0, " + std::to_string(B) + ")");
                track.indices.push_back((int32_t)b);
                track.weights.push_back(wi.at(k).as_float((ww + "[" + std::to_string(v) + "]").c_str()));
            }
        }
        const std::string pw = where + ".poses";
        if (!tr.at("poses").is_array() || tr.at("poses").size() != F)
            throw JsonError(pw + ": expected animation.frames (" + std::to_string(F) + ") palettes of " + std::to_string(B) + " matrices of 12 numbers");
        for (size_t f = 0; f < F; f++) {
            const Json &pal = tr.at("poses").at(f);
            const std::string fw = pw + "[" + std::to_string(f) + "]";
            if (!pal.is_array() || (long long)pal.size() != B) throw JsonError(fw + ": expected skin.bones (" + std::to_string(B) + ") matrices of 12 numbers");
            for (size_t b = 0; b < (size_t)B; b++) {
                const Json &m = pal.at(b);
                const std::string bw = fw + "[" + std::to_string(b) + "]";
                if (!m.is_array() || m.size() != 12) throw JsonError(bw + ": expected 12 numbers (a row-major 3 x 4 matrix)");
                for (size_t k = 0; k < 12; k++) {
                    const float v = m.at(k).as_float(bw.c_str());
                    if (!std::isfinite(v)) throw JsonError(bw + ": entry " + std::to_string(k) + " is not a finite fp32 number");
                    track.matrices.push_back(v);
                }
            }
        }
        track.bones = (int32_t)B;
    }
    std::vector<Track> tracks;
    double policy_ratio = 0.0; int policy_builder = -1; int rotations = 0; uint32_t rng_advance = 0;
    int frame = 0; float refit_ms = 0.f; int last_action = 0; double cost_ratio = 0.0;
};
} // namespace

// The reference's ground-truth technique: unidirectional path tracing with next-event estimation, one sample per
// pixel per iteration ("numSamplePerPixel" is read and unused, rtpt2.h:109).
class PathTraceTechnique {
public:
    // rtpt2.h:84-116
    void render(const HostScene &scene, int res_x, int res_y, const Json &json, const std::string &out_dir, int device) {
        rng_offset = (uint32_t)json.at("rngOffset").as_int("rngOffset");
        num_max_iteration = (int)json.at("numMaxIteration").as_int("numMaxIteration");
        time_limit_ms = json.at("timeLimitMs").as_float("timeLimitMs");
        {
            const std::string &fm = json.at("frameMode").as_string("frameMode");
            auto it = kFrameModes.find(fm);
            if (it == kFrameModes.end()) throw JsonError("frameMode: unknown value \"" + fm + "\"");
            frame_mode = it->second;
        }
        output_filename = output_path(out_dir, json.at("outputFilename").as_string("outputFilename"));
        stat_filename = output_path(out_dir, json.at("statFilename").as_string("statFilename"));
        use_jitter = json.at("useJitter").as_bool("useJitter");
        use_stat = json.at("useStat").as_bool("useStat");
        (void)json.at("numSamplePerPixel").as_int("numSamplePerPixel");
        num_max_bounce = (int)json.at("numMaxBounces").as_int("numMaxBounces");
        write_every_frame = json.has("writeEveryFrame") ? json.at("writeEveryFrame").as_bool("writeEveryFrame") : false;
        int bvh_builder = EVPLP_BVH_SAH;
        if (json.has("bvhBuilder")) bvh_builder = parse_bvh_builder(json.at("bvhBuilder").as_string("bvhBuilder"));
        conv.parse(json, out_dir, out_dir, res_x, res_y);
        denoise.parse(json, out_dir, frame_mode);
        // (before Noise::parse, as Denoise::parse: a "cleareveryframe" run with both blocks is refused under this block's name)
        if (frame_mode == 2 && json.has("adaptiveSampling")) throw JsonError("adaptiveSampling: frameMode \"cleareveryframe\" keeps no running sum");
        noise.parse(json, out_dir, out_dir, res_x, res_y, frame_mode);
        if (json.has("adaptive")) throw JsonError("adaptive: not for pt (VPL and VSL gathers only; pt takes \"adaptiveSampling\")");
        adaptive.parse(json, out_dir, frame_mode, false, run_options(json).shard_iterations, noise);                // build-only key "adaptiveSampling"
        // build-only key "samplesPerCall": S iterations per evplp_group_path_trace_batch call (default 1: the loop below as it always was).
        // Folds and retirements must fall on the iteration numbers they have with S = 1 -- a run is then the same bits for every S -- so
        // batchIterations (and with it everyIterations of both blocks, its multiples) must be a multiple of S
        if (json.has("samplesPerCall")) {
            const long long spc = json.at("samplesPerCall").as_int("samplesPerCall");
            if (spc < 1 || spc > 64) throw JsonError("samplesPerCall: must be 1 .. 64");
            samples_per_call = (int)spc;
        }
        adaptive.parse_budget_samples(samples_per_call);
        anim.parse(json, scene, time_limit_ms, num_max_iteration);                                                 // build-only key "animation"
        if (samples_per_call > 1) {
            if (frame_mode == 2) throw JsonError("samplesPerCall: frameMode \"cleareveryframe\" shows single samples (a batch always accumulates)");
            if (write_every_frame) throw JsonError("samplesPerCall: writeEveryFrame needs every iteration's frame (use samplesPerCall 1)");
            if (noise.on && noise.batch_iterations() % samples_per_call != 0)
                throw JsonError(std::string("samplesPerCall: noise.batchIterations") + (adaptive.on ? " (adaptiveSampling folds with it)" : "") + " must be a multiple of it");
        }

        evplp_config cfg; std::memset(&cfg, 0, sizeof(cfg));
        cfg.abi_version = EVPLP_ABI_VERSION; cfg.device = device; cfg.res_x = res_x; cfg.res_y = res_y;
        cfg.strip_rank = 0; cfg.strip_count = 1; cfg.strip_rows = 8;
        cfg.num_light_paths = 1; cfg.num_vpl_light_paths = 1; cfg.photons_per_path = 1;   // no light sub-paths in this technique
        cfg.bvh_builder = bvh_builder;
        Grp grp; create_group(grp, cfg, json, device);
        upload_scene_group(grp.g, scene);
        conv.upload(grp.g);
        anim.start(grp.g);
        denoise.start(grp.g);
        // "animation": every frame starts from the blocks as parsed, with its own file names
        const Convergence conv0 = conv; const Noise noise0 = noise; const Denoise denoise0 = denoise; const Adaptive adaptive0 = adaptive;
        const std::string output0 = output_filename, stat0 = stat_filename;
        const uint32_t rng_offset0 = rng_offset;
        for (int f = 0; f < anim.frames; f++) {
            if (anim.on) {
                anim.begin_frame(grp.g, f);
                rng_offset = anim.frame_rng_offset(rng_offset0, f);
                auto name = [&](const std::string &p) { return anim.frame_path(p); };
                conv = conv0; noise = noise0; denoise = denoise0; adaptive = adaptive0;
                conv.name_files(name); noise.name_files(name); denoise.name_files(name); adaptive.name_files(name);
                output_filename = name(output0); stat_filename = name(stat0);
            }
            run(grp.g, scene, res_x, res_y);
        }
    }

private:
    // rtpt2.h:575-719
    void run(evplp_group *h, const HostScene &scene, int W, int H) {
        JitterSampler sampler(rng_offset);
        check(h, evplp_group_clear_accumulators(h), "clear");
        noise.start(h, 1);
        adaptive.start(h, W, H, noise);
        int num_iterations = 0;
        auto t0 = std::chrono::steady_clock::now();
        auto elapsed_ms = [&]() { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        std::vector<float> rgb((size_t)W * H * 3);
        const bool clear_every_frame = frame_mode == 2;
        // samplesPerCall > 1: a batch of S iterations per call -- the same jitter stream and seeds as the loop below; the last batch is trimmed
        // at numMaxIteration; the time limit and the checkpoints are looked at once per batch (a convergence checkpoint that falls inside a
        // batch is taken at the batch's end, under that iteration number; folds and retirements fall on batch ends by construction)
        while (samples_per_call > 1) {
            if (num_iterations >= num_max_iteration) break;
            const int n = std::min(samples_per_call, num_max_iteration - num_iterations);
            float jitters[64][2] = {}; uint32_t seeds[64];
            for (int i = 0; i < n; i++) {
                if (use_jitter) sampler.next_jitter(W, H, jitters[i]);
                seeds[i] = (uint32_t)(num_iterations + i) + rng_offset;
            }
            check(h, evplp_group_path_trace_batch(h, scene.camera.origin, n, &jitters[0][0], seeds, (uint32_t)num_max_bounce), "path trace batch");
            const int first = num_iterations + 1;
            num_iterations += n;
            if (time_limit_ms < 1e8f) check(h, evplp_group_synchronize(h), "sync");
            bool conv_due = false;
            for (int i = first; i <= num_iterations && !conv_due; i++) conv_due = conv.due(i, elapsed_ms());
            if (conv_due) {
                const Composite k = composite(num_iterations);
                if (conv.checkpoint(h, num_iterations, [&] { check(h, evplp_group_synchronize(h), "sync"); return (double)elapsed_ms(); }, k.vs, k.ps, k.ls, k.mask_emitter)) break;
            }
            if (noise.on) {
                bool folded = false;
                for (int i = 0; i < n; i++) folded = noise.after_iteration(h, 0) || folded;       // (a fold can only fall on the batch's last iteration)
                const Composite k = composite(num_iterations);
                adaptive.after_fold(h, num_iterations, folded, k.vs, noise);
                if (noise.due(num_iterations, elapsed_ms(), folded) &&
                    noise.checkpoint(h, num_iterations, [&] { check(h, evplp_group_synchronize(h), "sync"); return (double)elapsed_ms(); }, k.vs, k.ls, k.mask_emitter)) break;
                if (adaptive.all_retired(noise)) break;
            }
            if (elapsed_ms() >= time_limit_ms) break;
        }
        if (samples_per_call <= 1) for (;;) {
            if (num_iterations == num_max_iteration) break;                                   // :610-613
            float jitter[2] = { 0.f, 0.f };
            if (use_jitter) sampler.next_jitter(W, H, jitter);                                // :618-624
            check(h, evplp_group_primary(h, jitter, clear_every_frame ? (EVPLP_LIGHT_CLEAR | EVPLP_LIGHT_UNOCCLUDED) : 0), "primary");        // :626-629, 633-643
            check(h, evplp_group_path_trace(h, scene.camera.origin, (uint32_t)num_iterations + rng_offset, (uint32_t)num_max_bounce,
                                            clear_every_frame ? 0 : 1), "path trace");       // :631
            num_iterations++;
            if (write_every_frame) {                                                          // :669-689
                size_t i = output_filename.find_last_of('.');
                save(h, W, H, num_iterations, output_filename.substr(0, i) + "_" + std::to_string(num_iterations) + output_filename.substr(i), rgb);
            }
            if (time_limit_ms < 1e8f) check(h, evplp_group_synchronize(h), "sync");
            if (conv.due(num_iterations, elapsed_ms())) {
                const Composite k = composite(num_iterations);
                if (conv.checkpoint(h, num_iterations, [&] { check(h, evplp_group_synchronize(h), "sync"); return (double)elapsed_ms(); }, k.vs, k.ps, k.ls, k.mask_emitter)) break;
            }
            if (noise.on) {
                const bool folded = noise.after_iteration(h, 0);
                const Composite k = composite(num_iterations);
                adaptive.after_fold(h, num_iterations, folded, k.vs, noise);
                if (noise.due(num_iterations, elapsed_ms(), folded) &&
                    noise.checkpoint(h, num_iterations, [&] { check(h, evplp_group_synchronize(h), "sync"); return (double)elapsed_ms(); }, k.vs, k.ls, k.mask_emitter)) break;
                if (adaptive.all_retired(noise)) break;                                       // every tile retired: nothing left to sample
            }
            if (elapsed_ms() >= time_limit_ms) break;                                         // :667
        }
        check(h, evplp_group_synchronize(h), "sync");
        float time = elapsed_ms();
        { const Composite k = composite(num_iterations); conv.finish(h, num_iterations, elapsed_ms(), k.vs, k.ps, k.ls, k.mask_emitter);
          noise.finish(h, num_iterations, elapsed_ms(), k.vs, k.ls, k.mask_emitter, W, H);
          denoise.accumulate(h, W, H, noise.batch_count(), k.vs, k.ls, k.mask_emitter); }
        if (use_stat) {                                                                       // :694-704
            Json st = Json::object();
            st.set("time", Json::number(time)); st.set("numIterations", Json::number(num_iterations));
            add_pass_times(h, st);
            anim.add_stat(st);
            denoise.add_stat(st);
            std::ofstream of(stat_filename);
            if (!of) throw std::runtime_error("cannot write " + stat_filename);
            of << st.dump() << "\n";
        }
        save(h, W, H, num_iterations, output_filename, rgb);                                  // :706-719
        adaptive.finish(h, num_iterations, W, H);
        { const Composite k = composite(num_iterations); denoise.write(h, W, H, noise.batch_count(), k.vs, k.ls, k.mask_emitter); }
    }
    // clear-every-frame: the composite as shown (masked emitter); accumulate: light image + path-traced image / n
    struct Composite { float vs, ps, ls; int32_t mask_emitter; };
    Composite composite(int n) const { return frame_mode == 2 ? Composite{ 1.0f, 0.0f, 1.0f, 1 } : Composite{ 1.0f / (float)std::max(n, 1), 0.0f, 1.0f, 0 }; }
    void save(evplp_group *h, int W, int H, int n, const std::string &path, std::vector<float> &rgb) {
        const Composite k = composite(n);
        check(h, evplp_group_resolve(h, k.vs, k.ps, k.ls, k.mask_emitter, 0, rgb.data()), "resolve");
        std::vector<float> top = flip_y(rgb, W, H);
        if (save_image(path.c_str(), W, H, top.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + path);
    }

    uint32_t rng_offset = 0; int num_max_iteration = 0, num_max_bounce = 0, frame_mode = 1, samples_per_call = 1;
    float time_limit_ms = 0.f;
    bool use_jitter = false, use_stat = false, write_every_frame = false;
    std::string output_filename, stat_filename;
    Convergence conv;
    Noise noise;
    Denoise denoise;
    Adaptive adaptive{"adaptiveSampling", true};
    Animation anim;
};

class ComPhotonTechnique {
public:
    // lvc: the "lvcphotonfam" twin (rtlvccomphoton.h).  It differs from RtComPhoton in the gather program
    // (per-pixel light-path window, lvclighttracing.cu:348-384), has no forceVsl / writeEveryFrame, and its stat
    // file carries only "time".
    explicit ComPhotonTechnique(bool lvc_variant = false) : lvc(lvc_variant) {}
    // rtcomphoton.h:107-223
    void render(const HostScene &scene, int res_x, int res_y, const Json &json, const std::string &out_dir, int device) {
        num_light_paths = (int)json.at("numLightPaths").as_int("numLightPaths");
        num_vpl_light_paths = (int)json.at("numVplLightPaths").as_int("numVplLightPaths");
        num_max_bounce = (int)json.at("numMaxBounces").as_int("numMaxBounces");
        photons_per_path = num_max_bounce + 1;
        radius_percentage = json.at("radiusPercentage").as_float("radiusPercentage");
        write_every_frame = (!lvc && json.has("writeEveryFrame")) ? json.at("writeEveryFrame").as_bool("writeEveryFrame") : false;
        num_max_iteration = (int)json.at("numMaxIteration").as_int("numMaxIteration");
        time_limit_ms = json.at("timeLimitMs").as_float("timeLimitMs");
        {
            const std::string &fm = json.at("frameMode").as_string("frameMode");
            auto it = kFrameModes.find(fm);
            if (it == kFrameModes.end()) throw JsonError("frameMode: unknown value \"" + fm + "\"");
            frame_mode = it->second;
        }
        if (!json.has("misMode")) mis_mode = 1;   // Balance (:128-131)
        else {
            const std::string &mm = json.at("misMode").as_string("misMode");
            auto it = kMisModes.find(mm);
            if (it == kMisModes.end()) throw JsonError("misMode: unknown value \"" + mm + "\"");
            mis_mode = it->second;
        }
        if (json.has("clampingStart"))            // :137-142
            throw JsonError("clampingStart option is not use anymore; remove it from your JSON file");
        if (json.has("targetRenderingTime")) target_rendering_time = json.at("targetRenderingTime").as_float("targetRenderingTime");
        rng_offset = (uint32_t)json.at("rngOffset").as_int("rngOffset");
        combined_filename = output_path(out_dir, json.at("combinedFilename").as_string("combinedFilename"));
        weighted_photon_filename = output_path(out_dir, json.at("weightedPhotonFilename").as_string("weightedPhotonFilename"));
        weighted_vpl_filename = output_path(out_dir, json.at("weightedVplFilename").as_string("weightedVplFilename"));
        stat_filename = output_path(out_dir, json.at("statFilename").as_string("statFilename"));
        use_jitter = json.at("useJitter").as_bool("useJitter");
        use_stat = json.at("useStat").as_bool("useStat");
        if (json.has("DoProgressive")) do_progressive = json.at("DoProgressive").as_bool("DoProgressive");
        if (json.has("AlphaProgressive")) alpha_progressive = json.at("AlphaProgressive").as_float("AlphaProgressive");
        if (json.has("run")) {                    // :188-197
            const Json &r = json.at("run");
            if (r.has("deferredShading")) do_deferred = r.at("deferredShading").as_bool("run.deferredShading");
            if (r.has("lightTracing")) do_light_tracing = r.at("lightTracing").as_bool("run.lightTracing");
            if (r.has("vplSplat")) do_vpl_splat = r.at("vplSplat").as_bool("run.vplSplat");
            if (r.has("photonSplat")) do_photon_splat = r.at("photonSplat").as_bool("run.photonSplat");
            if (r.has("lightRender")) do_light_render = r.at("lightRender").as_bool("run.lightRender");
            if (r.has("finalize")) do_finalize = r.at("finalize").as_bool("run.finalize");
        }
        if (num_vpl_light_paths == 0) { std::printf("WARN: 0 VPL light paths. Disable mDoVplSplat\n"); do_vpl_splat = false; }   // :200-203
        if (!lvc && json.has("forceVsl")) force_vsl = json.at("forceVsl").as_bool("forceVsl");
        if (json.has("bvhBuilder")) bvh_builder = parse_bvh_builder(json.at("bvhBuilder").as_string("bvhBuilder"));   // build-only key
        conv.parse(json, out_dir, out_dir, res_x, res_y);                                                          // build-only key
        denoise.parse(json, out_dir, frame_mode);                                                                   // build-only key
        noise.parse(json, out_dir, out_dir, res_x, res_y, frame_mode);                                             // build-only key
        anim.parse(json, scene, time_limit_ms, num_max_iteration);                                                 // build-only key

        // ---- setup(): context + scene upload (replaces GL/OptiX setup :646-708)
        evplp_config cfg; std::memset(&cfg, 0, sizeof(cfg));
        cfg.abi_version = EVPLP_ABI_VERSION; cfg.device = device; cfg.res_x = res_x; cfg.res_y = res_y;
        cfg.strip_rank = 0; cfg.strip_count = 1; cfg.strip_rows = 8;
        cfg.num_light_paths = (uint32_t)num_light_paths; cfg.num_vpl_light_paths = (uint32_t)num_vpl_light_paths;
        cfg.photons_per_path = (uint32_t)photons_per_path; cfg.bvh_builder = bvh_builder;
        if (json.has("deterministic")) cfg.deterministic = json.at("deterministic").as_bool("deterministic") ? 1 : 0;   // build-only key
        cfg.overlap_light_tracing = 1;      // the loop below calls primary, then light tracing: they overlap
        if (json.has("device")) {           // build-only: the bounds of the gathers' scratch buffers (evplp_config; defaults 8 GB / 2 GB)
            const Json &d = json.at("device");
            if (d.has("cutScratchGB")) cfg.cut_scratch_bytes = (uint64_t)(std::max(d.at("cutScratchGB").as_float("device.cutScratchGB"), 0.0f) * 1073741824.0);
            if (d.has("vslMaskGB")) cfg.vsl_mask_bytes = (uint64_t)(std::max(d.at("vslMaskGB").as_float("device.vslMaskGB"), 0.0f) * 1073741824.0);
        }
        run_opts = run_options(json);
        adaptive.parse(json, out_dir, frame_mode, lvc, run_opts.shard_iterations, noise, do_photon_splat && radius_percentage > 0.0f);   // build-only key
        const int gpus = device_gpus(json);
        if (run_opts.shard_iterations && (frame_mode != 1 || gpus < 2)) {
            if (gpus >= 2) std::printf("note: device.partition \"iterations\" needs frameMode \"accumulate\"; running on row strips\n");
            run_opts.shard_iterations = false;
        }
        // one group of N ranks: row strips, or whole-image ranks that share out the iterations
        Grp grp;
        create_group(grp, cfg, json, device, run_opts.shard_iterations);
        upload_scene_group(grp.g, scene);
        splat_footprint = setup_splat_footprint(grp.g, json, out_dir);                                           // :677
        conv.upload(grp.g);
        anim.start(grp.g);
        denoise.start(grp.g);
        // "animation": every frame starts from the blocks as parsed and from the moved scene's own figures, with its own file names
        const Convergence conv0 = conv; const Noise noise0 = noise; const Denoise denoise0 = denoise; const Adaptive adaptive0 = adaptive;
        const std::string combined0 = combined_filename, photon0 = weighted_photon_filename, vpl0 = weighted_vpl_filename, stat0 = stat_filename;
        const uint32_t rng_offset0 = rng_offset;
        for (int f = 0; f < anim.frames; f++) {
            if (anim.on) {
                anim.begin_frame(grp.g, f);
                rng_offset = anim.frame_rng_offset(rng_offset0, f);
                auto name = [&](const std::string &p) { return anim.frame_path(p); };
                conv = conv0; noise = noise0; denoise = denoise0; adaptive = adaptive0;
                conv.name_files(name); noise.name_files(name); denoise.name_files(name); adaptive.name_files(name);
                combined_filename = name(combined0); weighted_photon_filename = name(photon0); weighted_vpl_filename = name(vpl0); stat_filename = name(stat0);
            }
            float bsr = 0.f, total_area = 0.f, light_area = 0.f;
            { evplp_context *h0 = evplp_group_context(grp.g, 0);
              if (evplp_scene_metrics(h0, &bsr, &total_area, &light_area) < 0) throw std::runtime_error(std::string("scene metrics: ") + evplp_last_error(h0)); }

            photon_radius = bsr * radius_percentage;                                                                 // :118-119
            pdf_mc = (float)num_vpl_light_paths / (float)num_light_paths * kInvPi / (photon_radius * photon_radius); // :120
            if (!json.has("clampingCoeff")) {                                                                        // :148-161
                std::printf("Total area computation: %g\n", total_area);
                clamping_value = clamping_start = 1.f / total_area;
            } else clamping_value = clamping_start = json.at("clampingCoeff").as_float("clampingCoeff");
            if (force_vsl) {                                                                                         // :205-218
                float pct = json.at("vslRadiusPercentage").as_float("vslRadiusPercentage");
                vsl_radius = bsr * pct;
                if (vsl_radius <= 0.008f) { vsl_radius = std::max(vsl_radius, 0.008f); std::printf("warning : vslRadius is too small. clamped vslRadius\n"); }
                vsl_inv_pi_radius2 = kInvPi / (vsl_radius * vsl_radius);
            }
            run(grp.g, scene, res_x, res_y);
        }
    }

private:
    evplp_frame_params params(const HostScene &scene, uint32_t seed, const float jitter[2]) const {
        evplp_frame_params fp; std::memset(&fp, 0, sizeof(fp));
        std::memcpy(fp.camera_pos, scene.camera.origin, 12);
        fp.mis_mode = (uint32_t)mis_mode; fp.pdf_mc = pdf_mc; fp.clamping_value = clamping_value; fp.photon_radius = photon_radius;
        fp.vsl_radius = vsl_radius; fp.vsl_inv_pi_radius2 = vsl_inv_pi_radius2;
        fp.num_light_paths = (uint32_t)num_light_paths; fp.num_vpl_light_paths = (uint32_t)num_vpl_light_paths;
        fp.photons_per_path = (uint32_t)photons_per_path;
        fp.do_accumulate = frame_mode == 2 ? 0u : 1u;   // :923-930
        fp.rng_seed = seed; fp.jitter[0] = jitter[0]; fp.jitter[1] = jitter[1];
        fp.splat_footprint = splat_footprint;
        return fp;
    }

    // rtcomphoton.h:883-1133
    // h: one group of row-strip ranks, or of S ranks that share out the iterations (RunOptions::shard_iterations: iteration i on rank i % S)
    void run(evplp_group *h, const HostScene &scene, int W, int H) {
        JitterSampler sampler(rng_offset);
        const int S = run_opts.shard_iterations ? evplp_group_size(h) : 1;
        check(h, evplp_group_clear_accumulators(h), "clear");
        noise.start(h, 1);
        int num_iterations = 0;
        auto t0 = std::chrono::steady_clock::now();
        // Row blocks dealt by cost (RunOptions above): one frame of the first iteration's light paths and gather with the self-clocking
        // kernels, un-jittered, then the deal.  Nothing of it reaches the images: the rebalance clears the accumulators, the loop below traces
        // the same light paths again, the jitter sequence and the progressive state have not moved.  Its time is part of the run's.
        const bool can_deal = !run_opts.shard_iterations && evplp_group_size(h) > 1 && do_vpl_splat && !lvc && do_deferred && do_light_tracing;
        // (default: when the calibration frame pays for itself.  It costs one frame -- clocking a fraction of the VPLs deals worse than round robin,
        // measured -- and a dealt frame is ~1 % / ~4 % / ~20 % shorter than a round-robin one at 2 / 4 / 8 ranks, profiles/r06_strip_projection.json)
        const int ranks = evplp_group_size(h), pays_from = ranks >= 6 ? 5 : ranks >= 3 ? 25 : 100;
        if (can_deal && (run_opts.deal == 1 || (run_opts.deal < 0 && num_max_iteration >= pays_from))) {
            float j0[2] = { 0.f, 0.f };
            evplp_frame_params fp = params(scene, rng_offset, j0);
            check(h, evplp_group_calibrate(h, 1), "calibrate");
            check(h, evplp_group_primary(h, j0, EVPLP_LIGHT_SKIP), "primary (calibration)");
            check(h, evplp_group_trace_light_paths(h, rng_offset), "light tracing (calibration)");
            check(h, evplp_group_gather(h, &fp, force_vsl ? 1 : 0), "gather (calibration)");
            check(h, evplp_group_rebalance(h), "rebalance");
        }
        auto elapsed_ms = [&]() { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        // The wait in front of a look at the clock.  Strips: every rank (a frame is all of them).  Iterations: only the rank the NEXT iteration
        // reuses -- the others go on with theirs, and with S = 1 this is the same wait
        auto wait_for_next = [&]() {
            if (run_opts.shard_iterations) check(h, evplp_group_synchronize_rank(h, num_iterations % S), "sync");
            else check(h, evplp_group_synchronize(h), "sync");
        };
        float prev_timing = 0.f;
        std::vector<float> rgb((size_t)W * H * 3);
        // The two events per pass behind the stat file's pass times cost a sub-millisecond iteration ~3 % (evplp_profile_passes): a loop
        // that ends by iteration count records them in its last iteration only (a shard's: its last one); one with a time limit always.
        const bool always_profile = time_limit_ms < 1e8f;
        check(h, evplp_group_profile_passes(h, always_profile ? 1 : 0), "profile");
        bool profiling = always_profile;
        noise.start(h, S);
        adaptive.start(h, W, H, noise);
        for (;;) {
            if (num_iterations == num_max_iteration) break;                                   // :938-941
            if (run_opts.shard_iterations) check(h, evplp_group_select_rank(h, num_iterations % S), "select rank");   // (this iteration's rank)
            if (!profiling && num_iterations + S >= num_max_iteration) { check(h, evplp_group_profile_passes(h, 1), "profile"); profiling = true; }
            float jitter[2] = { 0.f, 0.f };
            if (use_jitter) sampler.next_jitter(W, H, jitter);                                // :946-952
            evplp_frame_params fp = params(scene, (uint32_t)num_iterations + rng_offset, jitter);
            const int light_flags = !do_light_render ? EVPLP_LIGHT_SKIP : frame_mode == 2 ? (EVPLP_LIGHT_CLEAR | EVPLP_LIGHT_UNOCCLUDED) : 0;   // :985-995
            // The reference draws the G-buffer first; the two passes are independent.  Pure photon mapping (no gather): light paths
            // first -- they start on the context's second stream, into the record buffer nobody reads, before the host has waited for
            // the previous iteration's photon bins.  With a gather in the frame they run beside the G-buffer pass instead of beside the
            // gather, whose CUs they would share.
            const bool light_first = !do_vpl_splat;
            if (light_first && do_light_tracing) check(h, evplp_group_trace_light_paths(h, (uint32_t)num_iterations + rng_offset), "light tracing");  // :962-966
            if (do_deferred) check(h, evplp_group_primary(h, jitter, light_flags), "primary");   // :954-960
            if (!light_first && do_light_tracing) check(h, evplp_group_trace_light_paths(h, (uint32_t)num_iterations + rng_offset), "light tracing");
            if (do_vpl_splat) check(h, evplp_group_gather(h, &fp, lvc ? 2 : force_vsl ? 1 : 0), "gather");  // :968-972
            // radius 0 (radiusPercentage 0 of the VPL-only configs): the proxy spheres are degenerate, nothing is drawn
            if (do_photon_splat && photon_radius > 0.0f) check(h, evplp_group_splat_photons(h, &fp, frame_mode == 2 ? 1 : 0), "photon splat");    // :974-983
            // [finalize] runFinalProgram(param, param, 1, true) to the window (:997-1004): headless, the composite still runs -- it is part
            // of the reference's iteration -- and stays on the device
            if (do_finalize) {
                const bool exchange = run_opts.exchange_every > 0 && (num_iterations + 1) % run_opts.exchange_every == 0;
                // (a rank's own frame: over ITS iterations so far; a reduction: over all of them)
                const float param = frame_mode == 2 ? 1.0f : 1.0f / (float)((exchange ? num_iterations : num_iterations / S) + 1);
                check(h, evplp_group_present_ex(h, param, param, 1.0f, 1, 1, exchange ? 1 : 0), "finalize");       // (doGammaCorrection = true, :1003)
            }
            num_iterations++;
            if (num_iterations % 20 == 0) {                                                   // :1008-1031
                wait_for_next();
                float cur = elapsed_ms();
                std::printf("numIter: %d | raduis: %g | clamping: %g | timing: %g\n", num_iterations, photon_radius, clamping_value, cur - prev_timing);
                if (target_rendering_time != -1.f) {
                    float frame_time = (cur - prev_timing) / 20.f, factor = target_rendering_time / frame_time;
                    if (factor != 1.f) std::printf("change number of samples: %g | currFrame time: %g\n", factor, frame_time);
                }
                prev_timing = cur;
            }
            if (do_progressive)                                                               // :1033-1063
                evplp_progressive_step(num_iterations, alpha_progressive, clamping_start, (uint32_t)num_vpl_light_paths, (uint32_t)num_light_paths,
                                       &photon_radius, &clamping_value, &pdf_mc, force_vsl ? 1 : 0, &vsl_radius, &vsl_inv_pi_radius2);
            if (write_every_frame) dump_frame(h, W, H, num_iterations, rgb);                  // :1079-1102
            if (time_limit_ms < 1e8f) wait_for_next();                                        // a wall-clock limit needs finished frames
            // the combinedFilename composite over ALL iterations so far (:1122; an iteration partition reduces the ranks' sums first)
            if (conv.due(num_iterations, elapsed_ms()) &&
                conv.checkpoint(h, num_iterations, [&] { wait_for_next(); return (double)elapsed_ms(); }, saved_param(num_iterations), saved_param(num_iterations), 1.0f, 0)) break;
            // (the fold of the rank this iteration ran on; the checkpoint, like conv's, measures the combinedFilename composite)
            if (noise.on) {
                const bool folded = noise.after_iteration(h, (num_iterations - 1) % S);
                adaptive.after_fold(h, num_iterations, folded, saved_param(num_iterations), noise);
                if (noise.due(num_iterations, elapsed_ms(), folded) &&
                    noise.checkpoint(h, num_iterations, [&] { wait_for_next(); return (double)elapsed_ms(); }, saved_param(num_iterations), 1.0f, 0)) break;
                if (adaptive.budget_spent(noise)) break;                                  // gather budget mode: every budget is 0
            }
            if (elapsed_ms() >= time_limit_ms) break;                                         // :1065
        }
        check(h, evplp_group_synchronize(h), "sync");                                         // (every iteration posted has finished)
        float time = elapsed_ms();
        conv.finish(h, num_iterations, elapsed_ms(), saved_param(num_iterations), saved_param(num_iterations), 1.0f, 0);
        noise.finish(h, num_iterations, elapsed_ms(), saved_param(num_iterations), 1.0f, 0, W, H);
        adaptive.finish(h, num_iterations, W, H);
        check(h, evplp_group_profile_passes(h, 1), "profile");
        denoise.accumulate(h, W, H, noise.batch_count(), saved_param(num_iterations), 1.0f, 0);
        if (use_stat) {                                                                       // :1109-1119
            Json st = Json::object();
            st.set("time", Json::number(time));
            if (!lvc) st.set("numIterations", Json::number(num_iterations));              // rtlvccomphoton.h writes the time only
            add_pass_times(h, st);
            anim.add_stat(st);
            denoise.add_stat(st);
            std::ofstream of(stat_filename);
            if (!of) throw std::runtime_error("cannot write " + stat_filename);
            of << st.dump() << "\n";
        }
        float param = saved_param(num_iterations);                                            // :1122
        // :1124-1132: three composites, un-masked sums, FlipY, Save (iterations: the first reduces, the other two composite the cached sums)
        auto compose = [&](float vs, float ps, float ls) {
            check(h, evplp_group_resolve(h, vs, ps, ls, 0, 0, rgb.data()), "resolve");
            return flip_y(rgb, W, H);
        };
        std::vector<float> combined = compose(param, param, 1.0f);
        std::vector<float> vpl = compose(param, 0.0f, 1.0f);
        std::vector<float> pm = compose(0.0f, param, 0.0f);
        if (save_image(combined_filename.c_str(), W, H, combined.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + combined_filename);
        if (save_image(weighted_vpl_filename.c_str(), W, H, vpl.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + weighted_vpl_filename);
        if (save_image(weighted_photon_filename.c_str(), W, H, pm.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + weighted_photon_filename);
        denoise.write(h, W, H, noise.batch_count(), param, 1.0f, 0);                         // (the combinedFilename composite, filtered)
    }

    float saved_param(int n) const { return frame_mode == 2 ? 1.0f : 1.0f / (float)std::max(n, 1); }     // :1122

    void dump_frame(evplp_group *h, int W, int H, int iter, std::vector<float> &rgb) {
        float param = frame_mode == 2 ? 1.0f : 1.0f / (float)iter;                            // :1088
        check(h, evplp_group_resolve(h, param, param, 1.0f, 0, 0, rgb.data()), "resolve");  // (iterations: the ranks' sums, reduced on the GPUs)
        std::vector<float> top = flip_y(rgb, W, H);
        size_t i = weighted_photon_filename.find_last_of('.');                                // :1097-1101
        std::string path = weighted_photon_filename.substr(0, i) + "_" + std::to_string(iter) + weighted_photon_filename.substr(i);
        if (save_image(path.c_str(), W, H, top.data()) != EVPLP_OK) throw std::runtime_error("cannot write " + path);
    }

    int num_light_paths = 0, num_vpl_light_paths = 0, num_max_bounce = 0, photons_per_path = 0;
    float radius_percentage = 0.f, photon_radius = 0.f, pdf_mc = 0.f;
    uint32_t rng_offset = 0; int num_max_iteration = 0; int frame_mode = 1; int mis_mode = 1;
    float time_limit_ms = 0.f, clamping_value = 0.f, clamping_start = 0.f;
    bool use_jitter = false, use_stat = false;
    bool do_deferred = true, do_light_tracing = true, do_vpl_splat = true, do_photon_splat = true, do_light_render = true, do_finalize = true;
    bool do_progressive = false, write_every_frame = false; float alpha_progressive = 0.7f;
    float target_rendering_time = -1.f;
    std::string combined_filename, weighted_photon_filename, weighted_vpl_filename, stat_filename;
    bool force_vsl = false; float vsl_radius = 0.f, vsl_inv_pi_radius2 = 0.f;
    bool lvc = false;
    uint32_t splat_footprint = EVPLP_FOOTPRINT_PROXY;
    RunOptions run_opts;
    Convergence conv;
    Noise noise;
    Adaptive adaptive;
    Denoise denoise;
    Animation anim;
    int bvh_builder = EVPLP_BVH_SAH;   // measured 9% faster frames than the Morton LBVH on the conference stand-in; "bvhBuilder": "lbvh" selects the LBVH
};

} // namespace evplp

extern "C" int evplp_jitter_sequence(uint32_t rng_offset, int32_t count, int32_t res_x, int32_t res_y, float *out_ndc_xy) {
    if (count < 0 || res_x <= 0 || res_y <= 0 || (count > 0 && !out_ndc_xy)) return EVPLP_ERR_INVALID;
    evplp::JitterSampler s(rng_offset);
    for (int32_t i = 0; i < count; i++) s.next_jitter(res_x, res_y, out_ndc_xy + 2 * (size_t)i);
    return EVPLP_OK;
}

// The product's JSON reader as the technique blocks use it (pinned against the reference's nlohmann::json 2.1.1 by
// tests/test_oracle_pins.py): `path` = keys separated by '/', decimal indices into arrays.  want: 0 int, 1 float, 2 bool,
// 3 string, 4 size, 5 kind (0 null, 1 bool, 2 number, 3 string, 4 array, 5 object).
// Returns 0 ok, 1 parse error, 2 key missing / index out of range, 3 conversion error.
extern "C" int evplp_json_query(const char *text, const char *path, int32_t want, double *num, char *str, int32_t cap) {
    using namespace evplp;
    if (!text || !path || !num) return EVPLP_ERR_INVALID;
    Json root;
    try { root = Json::parse(text); } catch (const std::exception &) { return 1; }
    const Json *j = &root;
    const std::string p(path);
    size_t at = 0;
    try {
        while (at < p.size()) {
            size_t e = p.find('/', at); if (e == std::string::npos) e = p.size();
            const std::string key = p.substr(at, e - at);
            at = e + 1;
            if (j->is_array()) { const size_t i = (size_t)std::stoul(key); if (i >= j->size()) return 2; j = &j->at(i); }
            else if (j->is_object()) { if (!j->has(key)) return 2; j = &j->at(key); }
            else return 2;
        }
    } catch (const std::exception &) { return 2; }
    try {
        switch (want) {
        case 0: *num = (double)(int)j->as_int(); break;
        case 1: *num = (double)j->as_float(); break;
        case 2: *num = j->as_bool() ? 1.0 : 0.0; break;
        case 3: { const std::string v = j->as_string(); if (!str || (int32_t)v.size() + 1 > cap) return 3; std::memcpy(str, v.data(), v.size()); str[v.size()] = 0; *num = (double)v.size(); break; }
        case 4: *num = (double)j->size(); break;
        default: *num = (double)j->kind(); break;
        }
    } catch (const std::exception &) { return 3; }
    return 0;
}

extern "C" int evplp_load_scene_json(evplp_context *ctx, const char *json_path) {
    using namespace evplp;
    if (!ctx || !json_path) return EVPLP_ERR_INVALID;
    try {
        Json root = Json::parse(read_text_file(json_path));
        HostScene scene = load_scene(root, json_path);
        return upload_scene(ctx, scene);
    } catch (const JsonError &e) { set_context_error(ctx, e.what()); return EVPLP_ERR_PARSE; }
    catch (const std::exception &e) { set_context_error(ctx, e.what()); return EVPLP_ERR_IO; }   // e.g. a Git-LFS pointer instead of a mesh, a missing file
}

extern "C" int evplp_render_json(const char *json_path, const char *json_overrides, int32_t device, char *err, size_t err_cap) {
    using namespace evplp;
    auto fail = [&](int code, const std::string &msg) { if (err && err_cap) { std::snprintf(err, err_cap, "%s", msg.c_str()); } return code; };
    if (!json_path) return fail(EVPLP_ERR_INVALID, "null json path");
    try {
        std::string text;
        try { text = read_text_file(json_path); } catch (const std::exception &e) { return fail(EVPLP_ERR_IO, e.what()); }
        Json root = Json::parse(text);                                                  // main.cpp:99-102
        HostScene scene;
        try { scene = load_scene(root, json_path); }                                    // main.cpp:104
        catch (const JsonError &e) { return fail(EVPLP_ERR_PARSE, e.what()); }
        catch (const std::exception &e) { return fail(EVPLP_ERR_IO, e.what()); }
        // every technique block that is present runs, in the reference's order (main.cpp:105-121)
        bool ran = false;
        auto block_of = [&](const char *key) {
            Json block = root.at(key);
            if (json_overrides && *json_overrides) block.merge(Json::parse(json_overrides));
            return block;
        };
        if (root.has("pt") && !root.at("pt").is_null()) {                               // main.cpp:105-109
            PathTraceTechnique t;
            t.render(scene, scene.res_x, scene.res_y, block_of("pt"), dirname_of(json_path), device);
            ran = true;
        }
        if (root.has("photonfam") && !root.at("photonfam").is_null()) {                 // main.cpp:111-115
            ComPhotonTechnique t;
            t.render(scene, scene.res_x, scene.res_y, block_of("photonfam"), dirname_of(json_path), device);
            ran = true;
        }
        if (root.has("lvcphotonfam") && !root.at("lvcphotonfam").is_null()) {           // main.cpp:117-121
            ComPhotonTechnique t(/*lvc_variant=*/true);
            t.render(scene, scene.res_x, scene.res_y, block_of("lvcphotonfam"), dirname_of(json_path), device);
            ran = true;
        }
        if (!ran) return fail(EVPLP_ERR_PARSE, "no technique block (\"pt\", \"photonfam\", \"lvcphotonfam\") in the scene JSON");
    } catch (const JsonError &e) { return fail(EVPLP_ERR_PARSE, e.what()); }
    catch (const IoError &e) { return fail(EVPLP_ERR_IO, e.what()); }
    catch (const InvalidError &e) { return fail(EVPLP_ERR_INVALID, e.what()); }
    catch (const std::exception &e) { return fail(EVPLP_ERR_HIP, e.what()); }
    return EVPLP_OK;
}
