// Primary visibility of one pixel -- ray set-up, the two packet walks, the four G-buffer texels and light_visible -- as a TEXT FRAGMENT
// included inside the body of primary_kernel (kernels_trace.hip) and of pt_batch_primary_kernel (kernels_ptbatch_primary.hip,
// evplp_path_trace_batch), so that the two are the same arithmetic.  A fragment and not a function: as an inlined function (by value, by
// reference, as a template) the code came out of the optimiser in another order and primary_kernel lost its instruction stream
// (compared with hipcc -S --cuda-device-only); included as text, its stream is what it was before the body moved here.
// Both translation units are built with -ffp-contract=off: the texels' bits depend on helpers inlined below (material_at, normalize_exact)
// that a lexical `#pragma clang fp contract(off)` in the kernel does not reach.
//   in scope at the include: PrimaryArgs a; int tx, ty, x, y; bool in_image (no early return before it: the walks are wave-collective)
//   macros: PRIMARY_JIT0, PRIMARY_JIT1 (the jitter), PRIMARY_USE_CUT (walk from the eye's entry cuts, not from the root)
//   declares: float4 pos, nrm, dif, phg; bool light_visible (and the locals of the walks)
// (no include guard: a fragment)
    // ray set-up and the hit point are written without fused multiply-adds, in the oracle's operation order: together
    // with the exact closest hit the G-buffer POSITIONS are then bit-identical to the CPU restatement, and so is every
    // threshold test downstream that reads them (the photon radius test |X_p - X|^2 <= r^2, frag:152-154)
    V3 eye = v3(a.cam.eye), S = v3(a.cam.s), U = v3(a.cam.u), F = v3(a.cam.f);
    float cx = ((float)x + 0.5f) / (float)a.st.W * 2.0f - 1.0f;
    float cy = ((float)y + 0.5f) / (float)a.st.H * 2.0f - 1.0f;
    // jittered matrix for the scene, original matrix for the light mesh (rtcomphoton.h:720-727)
    float jx = (cx - PRIMARY_JIT0) * a.cam.aspect * a.cam.tan_half, jy = (cy - PRIMARY_JIT1) * a.cam.tan_half;
    float ox = cx * a.cam.aspect * a.cam.tan_half, oy = cy * a.cam.tan_half;
    // (component-wise: the V3 operators are compiled with contraction allowed and would fuse after inlining)
    V3 dj = v3((S.x * jx + U.x * jy) + F.x, (S.y * jx + U.y * jy) + F.y, (S.z * jx + U.z * jy) + F.z);
    V3 d0 = v3((S.x * ox + U.x * oy) + F.x, (S.y * ox + U.y * oy) + F.y, (S.z * ox + U.z * oy) + F.z);

    float t = 0.f, b = 0.f, g = 0.f, tl = 0.f, bl = 0.f, gl = 0.f;
    // the 64 primary rays of a tile share the eye: packet walk (closest_wave), no per-lane stack.
    // view depth == t because the camera-space z of the direction is -1: near/far = [0.1, 100] (rtcommon.h:586)
    // the tile group's entry cut from the eye (primary_cut_kernel, once per camera: kernels.h PrimaryCutArgs), or the root
    const char *cut = nullptr;
    if (PRIMARY_USE_CUT) cut = a.cuts + (size_t)((ty >> a.cut_gh_log2) * a.cut_groups_x + (tx >> a.cut_gw_log2)) * (size_t)kCutSlotBytes;
    int32_t tri = closest_wave(a.sc, eye, dj, 0.1f, 100.0f, 1, in_image, t, b, g, cut);
    // the light mesh only matters in front of (or at) the scene hit (depth LEQUAL): bound its walk by that depth --
    // both directions have camera-space z = -1, so t is the view depth on either ray
    const bool light_unoccluded = (a.clear_light & EVPLP_LIGHT_UNOCCLUDED) != 0;      // wave-uniform
    const float light_far = (tri >= 0 && !light_unoccluded) ? fminf(t * 1.000001f + 1.0e-30f, 100.0f) : 100.0f;
    // ... and only tiles with a ray through the (padded) bounds of the light mesh walk at all: the emitters cover a small
    // part of most views and this second walk otherwise costs as much as the first
    bool light_maybe = in_image;
    {
        float t0 = 0.1f, t1 = light_far;
        const float o[3] = { eye.x, eye.y, eye.z }, d[3] = { d0.x, d0.y, d0.z };
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (d[k] == 0.0f) { if (o[k] < a.sc.light_lo[k] || o[k] > a.sc.light_hi[k]) light_maybe = false; }
            else {
                const float inv = 1.0f / d[k], ta = (a.sc.light_lo[k] - o[k]) * inv, tb = (a.sc.light_hi[k] - o[k]) * inv;
                t0 = fmaxf(t0, fminf(ta, tb) * 0.99999f - 1.0e-6f); t1 = fminf(t1, fmaxf(ta, tb) * 1.00001f + 1.0e-6f);
            }
        }
        if (t0 > t1) light_maybe = false;
    }
    const bool walk_light = a.sc.light_count > 0 && __ballot(light_maybe) != 0ull;        // wave-uniform
    int32_t ltri = walk_light ? closest_wave(a.sc, eye, d0, 0.1f, light_far, 2, in_image, tl, bl, gl, cut) : -1;
    bool use_light = ltri >= 0 && (tri < 0 || tl <= t);  // depth LEQUAL, light mesh drawn last
    const bool light_visible = light_unoccluded ? ltri >= 0 : use_light;              // the emitter IMAGE (rtcomphoton.h:985-995)
    if (use_light) { tri = ltri; b = bl; g = gl; }

    float4 pos = make_float4(0.f, 0.f, 0.f, 1.f);  // clear colour (0,0,0,1) rtcomphoton.h:885
    float4 nrm = make_float4(0.f, 0.f, 0.f, 0.f), dif = nrm, phg = nrm;
    if (tri >= 0) {
        const TriAttr &ta = a.sc.attrs[tri];
        V3 p0 = v3(ta.v), p1 = v3(ta.v + 3), p2 = v3(ta.v + 6);
        const float w0 = 1.0f - b - g;
        V3 P = v3((p1.x * b + p2.x * g) + p0.x * w0, (p1.y * b + p2.y * g) + p0.y * w0, (p1.z * b + p2.z * g) + p0.z * w0);
        V3 N = normalize_exact(cross_exact(p1 - p0, p2 - p0));  // deferred.geom:16-18 flat winding normal; the oracle's roundings: the
                                                                // sign of n1 . v12 decides which pairs trace a shadow ray (lighttracing.cu:284-288)
        V3 kd, ks; float ns;
        material_at(a.sc, ta, b, g, kd, ks, ns);
        pos = make_float4(P.x, P.y, P.z, 1.0f);
        nrm = make_float4(N.x, N.y, N.z, 0.f);
        dif = make_float4(kd.x, kd.y, kd.z, 0.f);
        phg = make_float4(ks.x, ks.y, ks.z, ns);
    }
