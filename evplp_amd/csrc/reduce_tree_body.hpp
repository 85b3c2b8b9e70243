// The balanced-tree sum of a pixel's per-group partials, as TEXT for the kernels that reduce a gather (kernels_gather.hip:
// gather_reduce_kernel and gather_reduce_budget_kernel), so that both sum in one order and neither kernel's code depends on the other.
// Expects: GatherArgs a; size_t i (the pixel); unsigned long long rays, shaded (the item statistics are added to them).  Leaves V3 r, the sum.
        const int groups = kVplSplit / a.splits_per_wave;
        V3 r = v3(0.f, 0.f, 0.f), lv0 = r, lv1 = r, lv2 = r, lv3 = r, lv4 = r, lv5 = r, lv6 = r;
        for (int g = 0; g < groups; g++) {
            float4 q = a.partial[(size_t)g * a.partial_stride + i];
            const uint32_t st = __float_as_uint(q.w);
            rays += st & 0xffffu; shaded += st >> 16;
            r = v3(q.x, q.y, q.z);
            // binary counter over g (level j holds the sum of 2^j consecutive partials): merge while the low bits of g are ones
#define EV_MERGE(L, NEXT) if (((g >> L) & 1) == 0) lv##L = r; else { r = lv##L + r; NEXT }
            EV_MERGE(0, EV_MERGE(1, EV_MERGE(2, EV_MERGE(3, EV_MERGE(4, EV_MERGE(5, EV_MERGE(6, ;)))))))
#undef EV_MERGE
        }
