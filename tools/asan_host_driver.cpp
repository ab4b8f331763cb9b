// Host-side AddressSanitizer driver (tests/test_host_asan.py; `make -C motion-style-transfer_amd/csrc asan`).
// Runs on the CPU, no GPU needed: calls every pure-host entry point of include/ynet_hip.h over a sweep of shapes and
// every launching entry point with arguments its validation must reject (null pointers, empty / oversized shapes), so
// that the instrumented host code -- argument checks, dispatch and workspace arithmetic, error formatting -- executes
// under ASan.  Exit code 0 = every rejection came back as a status code with a message, and ASan saw nothing.
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include "../include/ynet_hip.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                                      \
    do {                                                                                         \
        const int rc_ = (call);                                                                  \
        const char* msg_ = ynet_last_error();                                                    \
        if (rc_ == 0 || msg_ == nullptr || strlen(msg_) == 0) {                                  \
            fprintf(stderr, "NOT REJECTED: %s (rc %d)\n", #call, rc_);                           \
            ++failures;                                                                          \
        }                                                                                        \
    } while (0)

int main() {
    if (ynet_abi_version() != 1) ++failures;
    long long acc = 0;
    for (int cout : {1, 12, 16, 17, 32, 48, 64, 65, 130})
        for (int cin : {1, 6, 14, 32, 65, 130})
            for (int k : {1, 3, 5})
                for (int mode : {0, 1}) acc += ynet_packed_weight_floats(cout, cin, k, mode);
    for (int b : {1, 2, 10, 16, 32, 128, 256})
        for (int h : {1, 3, 8, 16, 32, 64, 96, 256, 512})
            for (int w : {1, 5, 8, 16, 32, 50, 64, 160, 256, 512})
                for (int cout : {1, 12, 16, 32, 48, 64, 130}) {
                    acc += ynet_conv2d_workspace_floats(b, h, w, cout);
                    for (int k : {1, 3, 5}) {
                        acc += ynet_conv2d_plan(b, h, w, cout, k);
                        acc += ynet_conv2d_wgrad_workspace_floats(b, h, w, cout, 32, k);
                    }
                }
    {   // ynet_conv2d_wgrad_plan: the dispatch of ynet_conv2d_wgrad without a launch; what it says the launch writes fits the workspace formula
        const int one_src[6][4] = {{1}, {14}, {32}, {33}, {65}, {130}};
        const int cat2[2] = {6, 8}, cat4[4] = {16, 16, 8, 2};
        YnetWgradPlan p;
        auto sweep = [&](const int* sc, int nsrc, int cout, int k) {
            int cin = 0;
            for (int i = 0; i < nsrc; ++i) cin += sc[i];
            for (int b : {1, 2, 5, 12, 16, 768})
                for (int h : {1, 2, 4, 5, 10, 18, 34, 64, 128})
                    for (int w : {1, 4, 32, 35, 36, 64, 96, 100})
                        for (int flags = 0; flags < 8; ++flags) {      // masked, aligned, want_bias
                            if (ynet_conv2d_wgrad_plan(b, h, w, cout, sc, nsrc, k, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, &p) != 0 || p.kernel < 1 || p.kernel > 4 ||
                                p.nsplit < 1 || p.partial_floats <= 0 || p.partial_floats > ynet_conv2d_wgrad_workspace_floats(b, h, w, cout, cin, k)) {
                                fprintf(stderr, "conv2d_wgrad_plan: B %d %dx%d cin %d cout %d K %d flags %d: kernel %d nsplit %d, %lld floats\n", b, h, w, cin, cout, k, flags,
                                        p.kernel, p.nsplit, p.partial_floats);
                                ++failures;
                            }
                            acc += p.kernel + p.nsplit + p.seg + p.ct;
                        }
        };
        for (int k : {1, 3, 5})
            for (int cout : {1, 3, 16, 17, 32, 33, 65, 130}) {
                for (const int* sc : one_src) sweep(sc, 1, cout, k);
                sweep(cat2, 2, cout, k);
                sweep(cat4, 4, cout, k);
            }
        EXPECT_REJECT(ynet_conv2d_wgrad_plan(1, 4, 4, 4, cat2, 2, 7, 0, 1, 1, &p));        // kernel size 7
        EXPECT_REJECT(ynet_conv2d_wgrad_plan(1, 4, 4, 4, cat2, 9, 3, 0, 1, 1, &p));        // 9 sources
        EXPECT_REJECT(ynet_conv2d_wgrad_plan(1, 0, 4, 4, cat2, 2, 3, 0, 1, 1, &p));        // H = 0
        EXPECT_REJECT(ynet_conv2d_wgrad_plan(1, 4, 4, 4, cat2, 2, 3, 0, 1, 1, nullptr));   // no plan to fill
        EXPECT_REJECT(ynet_conv2d_wgrad_plan(1, 4, 4, 4, nullptr, 2, 3, 0, 1, 1, &p));
    }
    acc += ynet_bce_workspace_bytes() + ynet_pred_bce_workspace_bytes() + ynet_comm_handle_bytes();
    if (acc <= 0) ++failures;

    float dummy[4] = {0, 0, 0, 0};
    float* fp = dummy;
    const float* cfp = dummy;
    int one = 1, status = 0;
    long long bs = 4;
    const float* srcs[1] = {cfp};
    float* dsts[1] = {fp};
    const float* null_srcs[1] = {nullptr};
    EXPECT_REJECT(ynet_pack_weight(nullptr, fp, 4, 4, 3, 0, nullptr));
    EXPECT_REJECT(ynet_pack_weight(cfp, fp, 4, 4, 4, 0, nullptr));              // kernel size 4
    EXPECT_REJECT(ynet_pack_weight(cfp, fp, 4, 4, 3, 7, nullptr));              // mode 7
    EXPECT_REJECT(ynet_conv2d(srcs, &one, &bs, nullptr, 0, nullptr, 0, cfp, nullptr, dsts, &one, &bs, 1, 1, 4, 4, 3, 0, nullptr, 0, nullptr));   // no source
    EXPECT_REJECT(ynet_conv2d(srcs, &one, &bs, nullptr, 1, nullptr, 0, nullptr, nullptr, dsts, &one, &bs, 1, 1, 4, 4, 3, 0, nullptr, 0, nullptr)); // no filter
    EXPECT_REJECT(ynet_conv2d(null_srcs, &one, &bs, nullptr, 1, nullptr, 0, cfp, nullptr, dsts, &one, &bs, 1, 1, 4, 4, 3, 0, nullptr, 0, nullptr));
    EXPECT_REJECT(ynet_conv2d(srcs, &one, &bs, nullptr, 1, nullptr, 0, cfp, nullptr, dsts, &one, &bs, 1, 0, 4, 4, 3, 0, nullptr, 0, nullptr));    // B = 0
    EXPECT_REJECT(ynet_conv2d(srcs, &one, &bs, nullptr, 1, nullptr, 0, cfp, nullptr, dsts, &one, &bs, 9, 1, 4, 4, 3, 0, nullptr, 0, nullptr));    // 9 destinations
    EXPECT_REJECT(ynet_conv2d_add(srcs, &one, &bs, nullptr, 1, cfp, nullptr, fp, 32, 16, 1, 4, 4, 3, 1, nullptr, 16, 0, nullptr));      // no addend
    EXPECT_REJECT(ynet_conv2d_add(srcs, &one, &bs, nullptr, 1, cfp, nullptr, fp, 32, 16, 1, 8, 8, 3, 1, cfp, 16, 1, nullptr));          // a map the additive kernels do not serve
    for (int b : {1, 32, 256})
        for (int hw : {8, 32, 64, 256})
            for (int cout : {12, 32, 48, 64}) acc += ynet_conv2d_add_supported(b, hw, hw, cout, 3);
    EXPECT_REJECT(ynet_conv2d_pool(srcs, &one, &bs, 1, cfp, nullptr, fp, 4, 64, nullptr, 16, 1, 4, 4, 3, 1, nullptr));               // no pooled output
    EXPECT_REJECT(ynet_conv2d_pool(srcs, &one, &bs, 1, cfp, nullptr, fp, 4, 64, fp, 16, 1, 5, 4, 3, 1, nullptr));                    // odd H
    for (int b : {1, 32, 256})
        for (int hw : {8, 32, 64, 256})
            for (int c : {12, 32, 48, 64}) acc += ynet_conv2d_pool_supported(b, hw, hw, c, 3) + ynet_conv2d_pool_supported(b, hw + 1, hw, c, 3);
    EXPECT_REJECT(ynet_conv2d_dgrad_relu(cfp, 4, 64, nullptr, 0, cfp, fp, 4, 64, nullptr, 64, 1, 4, 4, 3, nullptr, 0, nullptr));     // no activation
    EXPECT_REJECT(ynet_conv2d_dgrad_relu(cfp, 4, 64, nullptr, 0, cfp, fp, 4, 64, cfp + 1, 64, 1, 4, 4, 3, nullptr, 0, nullptr));     // unaligned activation
    for (int b : {1, 32, 256})
        for (int hw : {8, 32, 64, 256})
            for (int c : {12, 32, 48, 64}) acc += ynet_conv2d_dgrad_relu_supported(b, hw, hw, c, 3) + ynet_conv2d_dgrad_relu_supported(b, hw, hw + 2, c, 3);
    for (int b : {1, 10, 32, 256})
        for (int hw : {8, 32, 64, 128, 256})
            for (int c : {12, 16, 32, 48, 64, 130}) acc += ynet_conv2d_relu_bits_words(b, hw, hw, c, 3) + ynet_conv2d_relu_bits_words(b, hw, hw + 2, c, 3) + ynet_conv2d_relu_bits_words(b, hw, hw, c, 5);
    EXPECT_REJECT(ynet_conv2d_relu_bits(srcs, &one, &bs, 1, cfp, nullptr, fp, 32, 64, nullptr, 8, 128, 128, 3, nullptr));                 // no mask words
    EXPECT_REJECT(ynet_conv2d_relu_bits(srcs, &one, &bs, 1, cfp, nullptr, fp, 64, 64, (unsigned*)dummy, 2, 16, 16, 3, nullptr));            // shape not served
    EXPECT_REJECT(ynet_conv2d_dgrad_relu_bits(cfp, 4, 64, nullptr, 0, cfp, fp, 32, 64, nullptr, 8, 128, 128, 3, nullptr));                 // no mask words
    EXPECT_REJECT(ynet_conv2d_dgrad_relu_bits(cfp, 4, 64, nullptr, 0, cfp, fp, 64, 64, (const unsigned*)dummy, 2, 16, 16, 3, nullptr));     // shape not served
    for (int b : {1, 10, 32, 256})
        for (int hw : {8, 32, 64, 128, 256, 512})
            for (int c : {8, 16, 24, 32, 48, 64}) acc += ynet_conv2d_winograd_supported(b, hw, hw, c, 32, 3) + ynet_conv2d_winograd_supported(b, hw, hw + 2, 32, c, 3) + ynet_conv2d_winograd_supported(b, hw, hw, c, c, 5) + ynet_winograd_filter_floats(c, c);
    EXPECT_REJECT(ynet_winograd_filter(nullptr, fp, 32, 32, 0, 32, nullptr));
    EXPECT_REJECT(ynet_winograd_filter(cfp, fp, 12, 32, 0, 32, nullptr));                                                             // cin not a multiple of 8
    EXPECT_REJECT(ynet_winograd_filter(cfp, fp, 32, 32, 32, 48, nullptr));                                                            // slice beyond the filter
    EXPECT_REJECT(ynet_conv2d_winograd(cfp, 32 * 65536, cfp, nullptr, fp, 32 * 65536, 32, 48, 32, 256, 256, 1, nullptr));               // cout not served
    EXPECT_REJECT(ynet_conv2d_winograd(cfp, 32 * 65536, cfp, nullptr, fp, 32 * 65536, 32, 32, 32, 250, 256, 1, nullptr));               // H not a multiple of 16
    EXPECT_REJECT(ynet_conv2d_winograd(cfp, 16 * 65536, cfp, nullptr, fp, 32 * 65536, 32, 32, 32, 256, 256, 1, nullptr));               // batch stride smaller than the image
    EXPECT_REJECT(ynet_conv2d_winograd(nullptr, 32 * 65536, cfp, nullptr, fp, 32 * 65536, 32, 32, 32, 256, 256, 1, nullptr));
    // the Winograd-native 1-bit ReLU mask
    for (int b : {0, 1, 10, 32})
        for (int hw : {8, 32, 250, 256}) acc += ynet_winograd_relu_bits_words(b, hw, hw) + ynet_winograd_relu_bits_words(b, hw, hw + 16);
    EXPECT_REJECT(ynet_conv2d_winograd_relu_bits(cfp, 32 * 65536, cfp, nullptr, fp, 32 * 65536, 32, 32, 256, 256, nullptr, nullptr));                    // no mask words
    EXPECT_REJECT(ynet_conv2d_winograd_relu_bits(cfp, 32 * 65536, cfp, nullptr, fp, 32 * 65536, 12, 32, 256, 256, (unsigned*)dummy, nullptr));           // cin not a multiple of 8
    EXPECT_REJECT(ynet_conv2d_winograd_relu_bits(cfp, 32 * 65536, cfp, nullptr, fp, 16 * 65536, 32, 32, 256, 256, (unsigned*)dummy, nullptr));           // output stride smaller than the image
    EXPECT_REJECT(ynet_conv2d_winograd_dgrad_relu_bits(cfp, 32 * 65536, cfp, fp, 32 * 65536, nullptr, 32, 32, 256, 256, nullptr));                      // no mask words
    EXPECT_REJECT(ynet_conv2d_winograd_dgrad_relu_bits(cfp, 32 * 65536, cfp, fp, 32 * 65536, (const unsigned*)dummy, 32, 32, 250, 256, nullptr));       // H not a multiple of 16
    EXPECT_REJECT(ynet_conv2d_winograd_dgrad_relu_bits(cfp, 32 * 65536, nullptr, fp, 32 * 65536, (const unsigned*)dummy, 32, 32, 256, 256, nullptr));   // no filters
    {
        const int cat3[3] = {32, 16, 1}, cat2[2] = {32, 32}, bad[2] = {32, 0};
        const long long bs3[3] = {32 * 65536, 16 * 65536, 65536};
        const float* s3[3] = {cfp, cfp, cfp};
        for (int b : {1, 10, 32})
            for (int hw : {32, 128, 256})
                acc += ynet_conv2d_winograd_cat_supported(b, hw, hw, cat3, 3, 32, 3) + ynet_conv2d_winograd_cat_supported(b, hw, hw, cat2, 2, 32, 3) +
                       ynet_conv2d_winograd_cat_supported(b, hw, hw, cat3, 3, 16, 3) + ynet_conv2d_winograd_cat_supported(b, hw, hw, bad, 2, 32, 3) +
                       ynet_winograd_filter_cat_floats(cat3, 3, 32);
        EXPECT_REJECT(ynet_winograd_filter_cat(cfp, fp, cat3, 4, 32, 0, 32, nullptr));                                                   // too many sources
        EXPECT_REJECT(ynet_winograd_filter_cat(cfp, fp, bad, 2, 32, 0, 32, nullptr));                                                    // an empty source
        EXPECT_REJECT(ynet_conv2d_winograd_cat(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, 16, 32, 256, 256, 1, nullptr));              // 16 outputs: not served
        EXPECT_REJECT(ynet_conv2d_winograd_cat(s3, cat2, bs3, 2, cfp, nullptr, fp, 32 * 65536, 32, 32, 256, 256, 1, nullptr));              // 64 inputs: too many filters for LDS
        EXPECT_REJECT(ynet_conv2d_winograd_cat(s3, cat3, bs3, 3, nullptr, nullptr, fp, 32 * 65536, 32, 32, 256, 256, 1, nullptr));          // no filters
        EXPECT_REJECT(ynet_conv2d_winograd_cat_add(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, 32, 32, 256, 256, 1, nullptr, 32 * 65536, 4, nullptr));   // no additive term
        EXPECT_REJECT(ynet_conv2d_winograd_cat_add(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, 32, 32, 256, 256, 1, cfp, 32 * 65536, -1, nullptr));      // negative modulus
        EXPECT_REJECT(ynet_conv2d_winograd_cat_relu_bits(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, 32, 256, 256, nullptr, 0, 0, nullptr, nullptr));              // no mask words
        EXPECT_REJECT(ynet_conv2d_winograd_cat_relu_bits(s3, cat2, bs3, 2, cfp, nullptr, fp, 32 * 65536, 32, 256, 256, nullptr, 0, 0, (unsigned*)dummy, nullptr));     // 64 inputs: too many filters for LDS
        EXPECT_REJECT(ynet_conv2d_winograd_cat_relu_bits(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, 32, 256, 256, cfp, 32 * 65536, -1, (unsigned*)dummy, nullptr)); // negative modulus
        EXPECT_REJECT(ynet_conv2d_winograd_cat_pool(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, nullptr, 32 * 16384, 32, 32, 256, 256, 1, nullptr));   // no pooled output
        EXPECT_REJECT(ynet_conv2d_winograd_cat_pool_code(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, fp, 32 * 16384, nullptr, 32, 256, 256, nullptr));   // no code plane
        EXPECT_REJECT(ynet_conv2d_winograd_cat_pool_code(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, nullptr, 32 * 16384, (unsigned char*)dummy, 32, 256, 256, nullptr));   // no pooled output
        EXPECT_REJECT(ynet_conv2d_winograd_cat_pool_code(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, fp, 16 * 16384, (unsigned char*)dummy, 32, 256, 256, nullptr));     // pooled stride too small
        EXPECT_REJECT(ynet_conv2d_winograd_cat_pool(s3, cat3, bs3, 3, cfp, nullptr, fp, 32 * 65536, fp, 16 * 16384, 32, 32, 256, 256, 1, nullptr));        // pooled stride too small
    }
    {   // the slice form (round 5)
        const int one64[1] = {64}, cat3[3] = {32, 64, 1}, bad[2] = {32, 0};
        const long long bs1[1] = {64 * 4096}, bs3[3] = {32 * 4096, 64 * 4096, 4096};
        const float* s1[1] = {cfp};
        const float* s3[3] = {cfp, cfp, cfp};
        for (int b : {1, 10, 32, 256})
            for (int hw : {32, 64, 128, 256})
                for (int co : {16, 32, 48, 64, 128})
                    acc += ynet_conv2d_winograd16_supported(b, hw, hw, one64, 1, co, 3) + ynet_conv2d_winograd16_supported(b, hw, hw, cat3, 3, co, 3) +
                           ynet_conv2d_winograd16_supported(b, hw, hw + 16, one64, 1, co, 3) + ynet_conv2d_winograd16_supported(b, hw, hw, bad, 2, co, 3) +
                           ynet_conv2d_winograd16_supported(b, hw, hw, one64, 1, co, 5) + ynet_winograd16_filter_floats(cat3, 3, co);
        EXPECT_REJECT(ynet_winograd16_filter(cfp, fp, cat3, 4, 64, 0, 64, nullptr));                                                     // too many sources
        EXPECT_REJECT(ynet_winograd16_filter(cfp, fp, one64, 1, 24, 0, 64, nullptr));                                                    // cout not a multiple of 16
        EXPECT_REJECT(ynet_winograd16_filter(cfp, fp, one64, 1, 64, 32, 64, nullptr));                                                   // slice beyond the filter
        EXPECT_REJECT(ynet_conv2d_winograd16(s3, cat3, bs3, 3, cfp, nullptr, fp, 64 * 4096, 64, 32, 64, 64, 1, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr));   // 97 -> 100 padded channels: too many filters for LDS
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, nullptr, fp, 64 * 4096, 48, 32, 64, 64, 1, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr));  // 48 outputs: not a divisor of an XCD's workgroups
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, nullptr, fp, 64 * 4096, 64, 32, 48, 64, 1, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr));  // H not a multiple of 32
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, nullptr, fp, 32 * 4096, 64, 32, 64, 64, 1, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr));  // output stride smaller than the image
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, nullptr, fp, 64 * 4096, 64, 32, 64, 64, 0, cfp, 64 * 4096, cfp, 64 * 4096, 0, nullptr, 0, nullptr));  // two epilogue variants
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, cfp, fp, 64 * 4096, 64, 32, 64, 64, 0, cfp, 64 * 4096, nullptr, 0, 0, nullptr, 0, nullptr));         // relu_of with a bias
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, nullptr, fp, 64 * 4096, 64, 32, 64, 64, 1, nullptr, 0, cfp, 64 * 4096, -1, nullptr, 0, nullptr));    // negative modulus
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, cfp, nullptr, fp, 64 * 4096, 64, 32, 64, 64, 1, nullptr, 0, nullptr, 0, 0, fp, 16 * 1024, nullptr));       // pooled stride too small
        EXPECT_REJECT(ynet_conv2d_winograd16(s1, one64, bs1, 1, nullptr, nullptr, fp, 64 * 4096, 64, 32, 64, 64, 1, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr));      // no filters
    }
    for (int b : {1, 10, 32})
        for (int hw : {32, 128, 256})
            for (int c : {16, 32, 64}) acc += ynet_upsample2x_conv2d_winograd_supported(b, hw, hw, c, 16, 3) + ynet_upsample2x_conv2d_winograd_supported(b, hw, hw + 8, 32, c, 3);
    EXPECT_REJECT(ynet_upsample2x_conv2d_winograd(cfp, 32 * 16384, cfp, nullptr, fp, 16 * 65536, 32, 32, 32, 256, 256, 0, nullptr));     // 32 outputs: not served
    EXPECT_REJECT(ynet_upsample2x_conv2d_winograd(cfp, 32 * 16384, cfp, nullptr, fp, 16 * 65536, 32, 16, 32, 250, 256, 0, nullptr));     // H not a multiple of 16
    EXPECT_REJECT(ynet_upsample2x_conv2d_winograd(cfp, 16 * 16384, cfp, nullptr, fp, 16 * 65536, 32, 16, 32, 256, 256, 0, nullptr));     // input stride smaller than the low-resolution image
    EXPECT_REJECT(ynet_upsample2x_conv2d_winograd(cfp, 32 * 16384, cfp, nullptr, fp, 8 * 65536, 32, 16, 32, 256, 256, 0, nullptr));      // output stride smaller than the image
    EXPECT_REJECT(ynet_upsample2x_conv2d_winograd(nullptr, 32 * 16384, cfp, nullptr, fp, 16 * 65536, 32, 16, 32, 256, 256, 0, nullptr));
    EXPECT_REJECT(ynet_conv2d_winograd_dgrad_relu(cfp, 32 * 65536, cfp, fp, 32 * 65536, nullptr, 32 * 65536, 32, 32, 32, 256, 256, nullptr));   // no activation
    EXPECT_REJECT(ynet_conv2d_winograd_dgrad_relu(cfp, 32 * 65536, cfp, fp, 32 * 65536, cfp, 16 * 65536, 32, 32, 32, 256, 256, nullptr));       // activation stride too small
    EXPECT_REJECT(ynet_conv2d_wgrad(srcs, &one, &bs, 1, nullptr, 0, nullptr, 0, fp, nullptr, fp, 1, 4, 4, 1, 3, nullptr));
    EXPECT_REJECT(ynet_conv2d_wgrad(srcs, &one, &bs, 7, cfp, 4, nullptr, 0, fp, nullptr, fp, 1, 4, 4, 1, 3, nullptr));
    EXPECT_REJECT(ynet_lora_compose(nullptr, cfp, cfp, 1.f, fp, 4, 4, 3, 1, nullptr));
    EXPECT_REJECT(ynet_lora_grad(cfp, cfp, cfp, 1.f, fp, nullptr, 4, 4, 3, 1, nullptr));
    EXPECT_REJECT(ynet_lora_compose_pack(cfp, cfp, cfp, 1.f, fp, fp, 4, 4, 2, 1, nullptr));
    EXPECT_REJECT(ynet_train_readout(cfp, 16, nullptr, 16, 0, cfp, fp, fp, fp, fp, 1, 1, 4, 4, 1.f, nullptr));           // no goal map
    EXPECT_REJECT(ynet_train_readout(cfp, 16, cfp, 16, 0, cfp, fp, fp, fp, fp, 1, 1, 4, 4, 0.f, nullptr));               // resize factor 0
    for (int cin : {1, 6, 14, 32, 33, 64, 65})
        for (int cout : {1, 16, 32, 64, 130})
            for (int r : {1, 4}) acc += ynet_lora_conv2d_wgrad_supported(cin, cout, 3, r, 64) + ynet_lora_conv2d_wgrad_preferred(cin, cout, 3, r, 64) + ynet_lora_conv2d_wgrad_workspace_floats(cin, cout);
    EXPECT_REJECT(ynet_lora_conv2d_wgrad(srcs, &one, &bs, 1, nullptr, 4, nullptr, 0, cfp, cfp, 1.f, fp, fp, fp, 1, 4, 4, 4, 3, 1, nullptr));   // no dy
    EXPECT_REJECT(ynet_lora_conv2d_wgrad(srcs, &one, &bs, 1, cfp, 4, nullptr, 0, cfp, cfp, 1.f, fp, fp, fp, 1, 4, 4, 4, 3, 4, nullptr));       // rank 4
    EXPECT_REJECT(ynet_lora_conv2d_wgrad(srcs, &one, &bs, 1, cfp, 4, nullptr, 0, cfp, cfp, 1.f, fp, fp, fp, 1, 4, 6, 4, 3, 1, nullptr));       // W % 4
    EXPECT_REJECT(ynet_lora_conv2d_wgrad(srcs, &one, &bs, 1, cfp, 4, nullptr, 0, cfp, cfp, 1.f, fp, fp, fp, 1, 32768, 16384, 4, 3, 1, nullptr)); // 2^31 bytes per source image
    EXPECT_REJECT(ynet_lora_compose_pack_multi(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT_REJECT(ynet_lora_compose_pack_multi(99, srcs, srcs, srcs, cfp, dsts, dsts, &one, &one, &one, &one, nullptr));
    EXPECT_REJECT(ynet_adam_step(nullptr, &one, (const long long*)dummy, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, nullptr));     // no table
    EXPECT_REJECT(ynet_adam_step((const long long*)dummy, &one, (const long long*)dummy, 1, 1, 1e-3, 1.5, 0.999, 1e-8, 0.0, 0, nullptr));   // beta1 >= 1
    EXPECT_REJECT(ynet_batch_sum(cfp, fp, 2, 6, 6, nullptr));           // n % 4
    EXPECT_REJECT(ynet_batch_sum(nullptr, fp, 2, 8, 8, nullptr));
    EXPECT_REJECT(ynet_maxpool2_fwd(nullptr, fp, 1, 4, 4, nullptr));
    EXPECT_REJECT(ynet_maxpool2_bwd(cfp, cfp, nullptr, 1, 4, 4, nullptr));
    EXPECT_REJECT(ynet_upsample2x_fwd(cfp, nullptr, 1, 2, 2, nullptr));
    EXPECT_REJECT(ynet_upsample2x_bwd(nullptr, fp, 1, 2, 2, nullptr));
    EXPECT_REJECT(ynet_upsample2x_bwd_relu(cfp, fp, nullptr, 1, 2, 2, nullptr));
    EXPECT_REJECT(ynet_avgpool_pyramid(cfp, dsts, 9, 1, 32, 32, nullptr));
    EXPECT_REJECT(ynet_bce_logits_fwd(cfp, cfp, 0, fp, fp, nullptr));
    EXPECT_REJECT(ynet_bce_logits_fwd_grad(cfp, nullptr, 4, 1.f, fp, fp, fp, nullptr));
    EXPECT_REJECT(ynet_maxpool2_bwd_add_code(nullptr, cfp, nullptr, nullptr, fp, 4, 8, 8, 1, nullptr));                          // no code plane
    EXPECT_REJECT(ynet_maxpool2_bwd_add_code((const unsigned char*)dummy, cfp, nullptr, nullptr, fp, 4, 7, 8, 1, nullptr));      // odd H
    EXPECT_REJECT(ynet_pred_bce(cfp, 4, cfp, nullptr, cfp, fp, fp, nullptr, nullptr, fp, 1, 4, 33, 4, 1.f, 0, nullptr));   // cout 33
    EXPECT_REJECT(ynet_pred_bce(cfp, 4, cfp, nullptr, cfp, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 6, 1.f, 0, nullptr));   // HW % 4
    EXPECT_REJECT(ynet_pred_bce(cfp, 4, cfp, nullptr, nullptr, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 4, 1.f, 0, nullptr));                            // no target
    EXPECT_REJECT(ynet_pred_bce_blob(cfp, 4096, cfp, nullptr, nullptr, cfp, 31, 400, 64, 64, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 1.f, 0, nullptr));    // no positions
    EXPECT_REJECT(ynet_pred_bce_blob(cfp, 4096, cfp, nullptr, cfp, nullptr, 31, 400, 64, 64, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 1.f, 0, nullptr));    // no blob table
    EXPECT_REJECT(ynet_pred_bce_blob(cfp, 4096, cfp, nullptr, cfp, cfp, 31, 16, 64, 64, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 1.f, 0, nullptr));         // template smaller than the window
    EXPECT_REJECT(ynet_pred_bce_blob(cfp, 4096, cfp, nullptr, cfp, cfp, 31, 400, 64, 62, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 1.f, 0, nullptr));        // W % 4
    EXPECT_REJECT(ynet_pred_bce_blob(cfp, 4096, cfp, nullptr, cfp, cfp, 0, 400, 64, 64, fp, fp, nullptr, nullptr, fp, 1, 4, 12, 1.f, 0, nullptr));         // empty blob
    EXPECT_REJECT(ynet_softargmax2d(nullptr, fp, 1, 1, 4, 2, 2, nullptr));
    EXPECT_REJECT(ynet_pred_softargmax(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 1, 32, 12, 16, 32, nullptr));
    EXPECT_REJECT(ynet_pred_softargmax(fp, 32 * 17 * 23, fp, nullptr, fp, fp, 1, 32, 12, 17, 23, nullptr));      /* H*W % 128 != 0 */
    if (ynet_pred_softargmax_supported(24, 12, 16, 32) || ynet_pred_softargmax_supported(32, 33, 16, 32) || !ynet_pred_softargmax_supported(32, 30, 256, 256)) { fprintf(stderr, "pred_softargmax_supported\n"); return 1; }
    if (ynet_pred_softargmax_workspace_floats(4, 256, 256) != 4ll * 32 * 128) { fprintf(stderr, "pred_softargmax workspace\n"); return 1; }
    EXPECT_REJECT(ynet_sigmoid_temp(cfp, fp, 1, 4, 4, &one, 9, 1.f, nullptr));
    EXPECT_REJECT(ynet_sigmoid_temp(cfp, fp, 1, 4, 4, &one, 1, 0.f, nullptr));
    EXPECT_REJECT(ynet_gather_patch(cfp, 8, 8, cfp, fp, 1, 16, 16, &status, nullptr));      // window larger than the template
    EXPECT_REJECT(ynet_heatmap_analytic(cfp, fp, 1, 4, 4, 8, 0, 0.0, nullptr, 0, &status, nullptr));
    EXPECT_REJECT(ynet_heatmap_analytic(cfp, fp, 1, 4, 4, 8, 1, 1.0, nullptr, 31, &status, nullptr));
    EXPECT_REJECT(ynet_kmeans2d(cfp, &one, fp, &status, 1, 20000, 4, 1e-3f, 10, nullptr));
    EXPECT_REJECT(ynet_kmeans2d(cfp, &one, fp, &status, 1, 100, 4, 0.f, 0, nullptr));        // tol <= 0 without a limit: could not end
    EXPECT_REJECT(ynet_kmeans2d(cfp, &one, fp, &status, 1, 100, 4, 1e-3f, -1, nullptr));
    EXPECT_REJECT(ynet_multinomial(cfp, 1, 4, 4, 99, 0, 0.f, 1ull, (long long*)dummy, &status, nullptr));
    EXPECT_REJECT(ynet_multinomial(cfp, 1, 4, 4, 1, 0, 2.f, 1ull, (long long*)dummy, &status, nullptr));
    EXPECT_REJECT(ynet_cws_prior(cfp, 4, 1, cfp, cfp, 1, 2, 2, 0.f, 1.f, 0, fp, fp, nullptr));
    EXPECT_REJECT(ynet_score_rank_samples(cfp, cfp, cfp, 2, 65, 1, 12, 8, 8, 4.f, fp, &status, fp, fp, &status, nullptr));      // K > 64
    EXPECT_REJECT(ynet_score_rank_samples(cfp, cfp, cfp, 2, 0, 1, 12, 8, 8, 4.f, fp, &status, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_score_rank_samples(cfp, cfp, cfp, 2, 20, 1, 12, 8, 8, 0.f, fp, &status, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_map_likelihood(nullptr, 16, cfp, 1, 1, 4, 4, 1.f, fp, fp, fp, &status, nullptr));                 // no map
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, 0.f, fp, fp, fp, &status, nullptr));                     // temperature 0
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, -1.f, fp, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, 1.f / 0.f, fp, fp, fp, &status, nullptr));               // not finite
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, 0.f / 0.f, fp, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, 1e-39f, fp, fp, fp, &status, nullptr));                  // a denormal: 1 / T overflows
    EXPECT_REJECT(ynet_map_likelihood(cfp, 1ll << 31, cfp, 1, 1, 32768, 65536, 1.f, fp, fp, fp, &status, nullptr));      // 2^31 pixels per plane
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 0, 1, 4, 4, 1.f, fp, fp, fp, &status, nullptr));                     // B, C, H, W < 1
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 0, 4, 4, 1.f, fp, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 0, 4, 1.f, fp, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 0, 1.f, fp, fp, fp, &status, nullptr));
    EXPECT_REJECT(ynet_map_likelihood(cfp, 31, cfp, 2, 2, 4, 4, 1.f, fp, fp, fp, &status, nullptr));                     // batch stride below the image
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, 1.f, nullptr, nullptr, nullptr, &status, nullptr));      // no output
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, nullptr, 1, 1, 4, 4, 1.f, fp, fp, nullptr, &status, nullptr));            // nll without the ground truth
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, nullptr, 1, 1, 4, 4, 1.f, nullptr, fp, fp, &status, nullptr));            // hpd without the ground truth
    EXPECT_REJECT(ynet_map_likelihood(cfp, 16, cfp, 1, 1, 4, 4, 1.f, fp, fp, fp, nullptr, nullptr));                     // ground truth without a status flag
    {
        const unsigned char* lab = reinterpret_cast<const unsigned char*>(dummy);
        EXPECT_REJECT(ynet_map_class_mass(nullptr, 16, lab, 0, 1, 1, 4, 4, 6, 1.f, fp, nullptr));                        // no map
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, nullptr, 0, 1, 1, 4, 4, 6, 1.f, fp, nullptr));                        // no labels
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 4, 6, 1.f, nullptr, nullptr));                       // no output
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 4, 0, 1.f, fp, nullptr));                            // n_classes outside 1 .. 8
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 4, YNET_MAP_MAX_CLASSES + 1, 1.f, fp, nullptr));
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 4, 6, 0.f, fp, nullptr));                            // temperature 0
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 4, 6, 0.f / 0.f, fp, nullptr));                      // not finite
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 4, 6, 1e-39f, fp, nullptr));                         // a denormal: 1 / T overflows
        EXPECT_REJECT(ynet_map_class_mass(cfp, 1ll << 31, lab, 0, 1, 1, 32768, 65536, 6, 1.f, fp, nullptr));             // 2^31 pixels per plane
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 0, 1, 4, 4, 6, 1.f, fp, nullptr));                            // B, C, H, W < 1
        EXPECT_REJECT(ynet_map_class_mass(cfp, 16, lab, 0, 1, 1, 4, 0, 6, 1.f, fp, nullptr));
        EXPECT_REJECT(ynet_map_class_mass(cfp, 31, lab, 0, 2, 2, 4, 4, 6, 1.f, fp, nullptr));                            // batch stride below the image
        EXPECT_REJECT(ynet_map_class_mass(cfp, 32, lab, 15, 2, 2, 4, 4, 6, 1.f, fp, nullptr));                           // label stride neither 0 nor a plane
        EXPECT_REJECT(ynet_map_class_mass(cfp, 4, lab, 0, 1ll << 29, 4, 1, 1, 6, 1.f, fp, nullptr));                     // 2^31 planes
    }
    {   // the credible levels are read on the host: exactly n_levels of them (heap arrays of that length, so a read past them is seen)
        float* q8 = new float[YNET_MAP_CREDIBLE_MAX_LEVELS];
        float* q2 = new float[2];
        for (int l = 0; l < YNET_MAP_CREDIBLE_MAX_LEVELS; ++l) q8[l] = 0.1f + 0.1f * l;
        q2[0] = 0.5f, q2[1] = 0.9f;
        int* ip = reinterpret_cast<int*>(dummy);
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 0, 1, 4, 4, q8, YNET_MAP_CREDIBLE_MAX_LEVELS, 1.f, ip, fp, fp, &status, nullptr));     // B < 1, found after all 8 were read
        EXPECT_REJECT(ynet_map_credible(nullptr, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, fp, &status, nullptr));                            // no map
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, nullptr, 2, 1.f, ip, fp, fp, &status, nullptr));                           // no levels
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, nullptr, fp, fp, &status, nullptr));                           // no outputs
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, nullptr, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, nullptr, &status, nullptr));
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, fp, nullptr, nullptr));                                // no status flag
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 0, 1.f, ip, fp, fp, &status, nullptr));                                // n_levels outside 1 .. 8
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, YNET_MAP_CREDIBLE_MAX_LEVELS + 1, 1.f, ip, fp, fp, &status, nullptr)); // (refused before a level is read)
        q2[1] = 0.5f;
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, fp, &status, nullptr));                                // not ascending strictly
        q2[1] = 1.f;
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, fp, &status, nullptr));                                // outside (0, 1)
        q2[0] = 0.f, q2[1] = 0.9f;
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, fp, &status, nullptr));
        q2[0] = 0.f / 0.f;
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1.f, ip, fp, fp, &status, nullptr));
        q2[0] = 0.5f;
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 0.f, ip, fp, fp, &status, nullptr));                                // temperature 0
        EXPECT_REJECT(ynet_map_credible(cfp, 16, 1, 1, 4, 4, q2, 2, 1e-39f, ip, fp, fp, &status, nullptr));                             // a denormal: 1 / T overflows
        EXPECT_REJECT(ynet_map_credible(cfp, 1ll << 23, 1, 1, 2048, 2049, q2, 2, 1.f, ip, fp, fp, &status, nullptr));                   // above the pixel cap
        EXPECT_REJECT(ynet_map_credible(cfp, 31, 2, 2, 4, 4, q2, 2, 1.f, ip, fp, fp, &status, nullptr));                                // batch stride below the image
        EXPECT_REJECT(ynet_map_credible(cfp, 4, 1ll << 22, 1, 1, 1, q2, 2, 1.f, ip, fp, fp, &status, nullptr));                         // too many planes
        delete[] q8;
        delete[] q2;
    }
    {   // scene occupancy: the refusals (the offsets are device data: the host never reads them), and the workspace arithmetic over a small sweep
        alignas(8) double wsbuf[1] = {0.0};
        void* ws = wsbuf;
        const int* off = &one;
        EXPECT_REJECT(ynet_map_occupancy(nullptr, 16, off, 1, 1, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));             // no map
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, nullptr, 1, 1, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));             // no offsets
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 1.f, nullptr, fp, fp, fp, ws, &status, nullptr));            // no occupancy
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, nullptr, &status, nullptr));            // no workspace
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, (char*)ws + 4, &status, nullptr));      // workspace off an 8-byte boundary
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, nullptr, nullptr));                 // no status flag
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 0, 1.f, fp, fp, fp, fp, ws, &status, nullptr));                 // cell outside {1, 2, 4, 8}
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 3, 1.f, fp, fp, fp, fp, ws, &status, nullptr));
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2 * YNET_MAP_OCCUPANCY_MAX_CELL, 1.f, fp, fp, fp, fp, ws, &status, nullptr));
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 0.f, fp, fp, fp, fp, ws, &status, nullptr));                 // temperature 0
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 0.f / 0.f, fp, fp, fp, fp, ws, &status, nullptr));           // not finite
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 4, 2, 1e-39f, fp, fp, fp, fp, ws, &status, nullptr));              // a denormal: 1 / T overflows
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 0, 1, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));                 // B, G, C, H, W < 1
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 0, 1, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 0, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 0, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));
        EXPECT_REJECT(ynet_map_occupancy(cfp, 16, off, 1, 1, 1, 4, 0, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));
        EXPECT_REJECT(ynet_map_occupancy(cfp, 31, off, 2, 1, 2, 4, 4, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));                 // batch stride below the image
        EXPECT_REJECT(ynet_map_occupancy(cfp, 1ll << 31, off, 1, 1, 1, 32768, 65536, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));  // 2^31 pixels per plane
        EXPECT_REJECT(ynet_map_occupancy(cfp, 4, off, 1ll << 29, 1, 4, 1, 1, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));          // 2^31 planes
        EXPECT_REJECT(ynet_map_occupancy(cfp, 4, off, 1, 1ll << 29, 4, 1, 1, 2, 1.f, fp, fp, fp, fp, ws, &status, nullptr));          // 2^31 (g, c, tile) workgroups
        const int cells[4] = {1, 2, 4, 8};
        for (int ci = 0; ci < 4; ++ci) {
            const int cell = cells[ci], pw = cell < 4 ? 4 : cell;
            for (int H = 1; H <= 33; H += 4) {
                for (int W = 1; W <= 70; W += 23) {
                    for (long long B = 1; B <= 9; B += 4) {
                        for (long long G = 1; G <= 3; ++G) {
                            const long long T = ((long long)((W + pw - 1) / pw) * ((H + cell - 1) / cell) + 63) / 64;
                            if (ynet_map_occupancy_workspace_bytes(B, 3, H, W, G, cell) != 8 * (B * 3 + G * 3 * T + B * 3 * T)) {
                                fprintf(stderr, "map_occupancy_workspace_bytes(%lld, 3, %d, %d, %lld, %d)\n", B, H, W, G, cell);
                                return 1;
                            }
                        }
                    }
                }
            }
        }
        if (ynet_map_occupancy_workspace_bytes(0, 3, 4, 4, 1, 2) != -1 || ynet_map_occupancy_workspace_bytes(1, 3, 4, 4, 1, 3) != -1
            || ynet_map_occupancy_workspace_bytes(1, 3, 4, 4, 0, 2) != -1 || ynet_map_occupancy_workspace_bytes(1, 1, 32768, 65536, 1, 1) != -1
            || ynet_map_occupancy_workspace_bytes(1ll << 29, 4, 1, 1, 1, 1) != -1 || ynet_map_occupancy_workspace_bytes(1, 4, 1, 1, 1ll << 29, 1) != -1) {
            fprintf(stderr, "map_occupancy_workspace_bytes: a refused shape got a size\n");
            return 1;
        }
    }
    {   // radial scores: the refusals (the ground truth is device data: the host never reads it)
        EXPECT_REJECT(ynet_map_radial(nullptr, 16, cfp, 1, 1, 4, 4, 1.f, 5, fp, fp, fp, fp, &status, nullptr));                       // no map
        EXPECT_REJECT(ynet_map_radial(cfp, 16, nullptr, 1, 1, 4, 4, 1.f, 5, fp, fp, fp, fp, &status, nullptr));                       // no ground truth
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 1.f, 5, nullptr, nullptr, nullptr, nullptr, &status, nullptr));       // no output
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 1.f, 5, fp, fp, fp, fp, nullptr, nullptr));                           // no status flag
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 1.f, 0, fp, fp, fp, fp, &status, nullptr));                           // n_rings outside 1 .. 1024
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 1.f, YNET_MAP_RADIAL_MAX_RINGS + 1, fp, fp, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 0.f, 5, fp, fp, fp, fp, &status, nullptr));                           // temperature 0
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 0.f / 0.f, 5, fp, fp, fp, fp, &status, nullptr));                     // not finite
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 4, 1e-39f, 5, fp, fp, fp, fp, &status, nullptr));                        // a denormal: 1 / T overflows
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 0, 1, 4, 4, 1.f, 5, fp, fp, fp, fp, &status, nullptr));                           // B, C, H, W < 1
        EXPECT_REJECT(ynet_map_radial(cfp, 16, cfp, 1, 1, 4, 0, 1.f, 5, fp, fp, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_radial(cfp, 1ll << 20, cfp, 1, 1, YNET_MAP_RADIAL_MAX_SIDE + 1, 1, 1.f, 5, fp, fp, fp, fp, &status, nullptr));   // a side above 16384
        EXPECT_REJECT(ynet_map_radial(cfp, 1ll << 23, cfp, 1, 1, 2048, 2049, 1.f, 5, fp, fp, fp, fp, &status, nullptr));              // above the pixel cap
        EXPECT_REJECT(ynet_map_radial(cfp, 31, cfp, 2, 2, 4, 4, 1.f, 5, fp, fp, fp, fp, &status, nullptr));                           // batch stride below the image
        EXPECT_REJECT(ynet_map_radial(cfp, 4, cfp, 1ll << 29, 4, 1, 1, 1.f, 5, fp, fp, fp, fp, &status, nullptr));                    // 2^31 planes
    }
    {   // marginals: the refusals (the ground truth is device data: the host never reads it)
        EXPECT_REJECT(ynet_map_marginals(nullptr, 16, cfp, 1, 1, 4, 4, 1.f, fp, fp, fp, fp, &status, nullptr));                       // no map
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 1, 1, 4, 4, 1.f, nullptr, nullptr, nullptr, nullptr, &status, nullptr));       // no output
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, nullptr, 1, 1, 4, 4, 1.f, fp, fp, fp, nullptr, &status, nullptr));                  // crps without a ground truth
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, nullptr, 1, 1, 4, 4, 1.f, fp, fp, nullptr, fp, &status, nullptr));                  // pit without one
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 1, 1, 4, 4, 1.f, fp, fp, fp, fp, nullptr, nullptr));                           // ... without a status flag
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 1, 1, 4, 4, 0.f, fp, fp, fp, fp, &status, nullptr));                           // temperature 0
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 1, 1, 4, 4, 0.f / 0.f, fp, fp, fp, fp, &status, nullptr));                     // not finite
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 1, 1, 4, 4, 1e-39f, fp, fp, fp, fp, &status, nullptr));                        // a denormal: 1 / T overflows
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 0, 1, 4, 4, 1.f, fp, fp, fp, fp, &status, nullptr));                           // B, C, H, W < 1
        EXPECT_REJECT(ynet_map_marginals(cfp, 16, cfp, 1, 1, 4, 0, 1.f, fp, fp, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_marginals(cfp, 1ll << 20, cfp, 1, 1, YNET_MAP_MARGINALS_MAX_SIDE + 1, 1, 1.f, fp, fp, fp, fp, &status, nullptr));   // a side above 2048
        EXPECT_REJECT(ynet_map_marginals(cfp, 1ll << 20, nullptr, 1, 1, 1, YNET_MAP_MARGINALS_MAX_SIDE + 1, 1.f, fp, fp, nullptr, nullptr, nullptr, nullptr));
        EXPECT_REJECT(ynet_map_marginals(cfp, 31, cfp, 2, 2, 4, 4, 1.f, fp, fp, fp, fp, &status, nullptr));                           // batch stride below the image
        EXPECT_REJECT(ynet_map_marginals(cfp, 4, cfp, 1ll << 29, 4, 1, 1, 1.f, fp, fp, fp, fp, &status, nullptr));                    // 2^31 planes
    }
    {   // the sweep reads its temperatures on the host: exactly n_temps of them (a heap array of that length, so a read past it is seen)
        float* t32 = new float[YNET_SWEEP_MAX_TEMPS];
        float* t3 = new float[3];
        for (int k = 0; k < YNET_SWEEP_MAX_TEMPS; ++k) t32[k] = 0.25f + 0.25f * k;
        t3[0] = 1.f, t3[1] = 1.8f, t3[2] = 0.f;
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 0, 1, 4, 4, t32, YNET_SWEEP_MAX_TEMPS, fp, fp, &status, nullptr));      // B < 1, found after all 32 were read
        EXPECT_REJECT(ynet_map_likelihood_sweep(nullptr, 16, cfp, 1, 1, 4, 4, t32, YNET_SWEEP_MAX_TEMPS, fp, fp, &status, nullptr));  // no map
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, nullptr, 3, fp, fp, &status, nullptr));            // no temperatures
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t32, 0, fp, fp, &status, nullptr));                // n_temps outside 1 .. 32
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t32, YNET_SWEEP_MAX_TEMPS + 1, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));                 // the last of three is 0
        t3[2] = -1.f;
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));
        t3[2] = 1.f / 0.f;
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));                 // not finite
        t3[2] = 0.f / 0.f;
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));
        t3[2] = 1e-39f;
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));                 // a denormal: 1 / T overflows
        t3[2] = 2.5f;
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 1ll << 31, cfp, 1, 1, 32768, 65536, t3, 3, fp, fp, &status, nullptr));  // 2^31 pixels per plane
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 0, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));                 // B, C, H, W < 1
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 0, 4, 4, t3, 3, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 0, 4, t3, 3, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 0, t3, 3, fp, fp, &status, nullptr));
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 31, cfp, 2, 2, 4, 4, t3, 3, fp, fp, &status, nullptr));                 // batch stride below the image
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, nullptr, nullptr, &status, nullptr));       // no output
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, nullptr, 1, 1, 4, 4, t3, 3, fp, fp, &status, nullptr));             // no ground truth
        EXPECT_REJECT(ynet_map_likelihood_sweep(cfp, 16, cfp, 1, 1, 4, 4, t3, 3, fp, fp, nullptr, nullptr));                 // no status flag
        delete[] t32;
        delete[] t3;
    }
    EXPECT_REJECT(ynet_map_modes(nullptr, 16, 1, 1, 4, 4, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));           // no map
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 1.f, nullptr, fp, fp, &status, &status, nullptr));          // no xy
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 1.f, fp, nullptr, fp, &status, &status, nullptr));          // no logit
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 1.f, fp, fp, fp, nullptr, &status, nullptr));               // no count
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 1.f, fp, fp, fp, &status, nullptr, nullptr));               // no status flag
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 0, 3, 1.f, fp, fp, fp, &status, &status, nullptr));                // n_modes outside 1 .. 64
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 65, 3, 1.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, -1, 1.f, fp, fp, fp, &status, &status, nullptr));              // radius < 0
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 0, 1, 4, 4, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));               // B, C, H, W < 1
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 0, 4, 4, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 0, 4, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 0, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 31, 2, 2, 4, 4, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));               // batch stride below the image
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 0.f, fp, fp, fp, &status, &status, nullptr));               // with mass: temperature 0
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, -1.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 1.f / 0.f, fp, fp, fp, &status, &status, nullptr));         // not finite
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 0.f / 0.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1, 1, 4, 4, 20, 3, 1e-39f, fp, fp, fp, &status, &status, nullptr));            // a denormal: 1 / T overflows
    EXPECT_REJECT(ynet_map_modes(cfp, 1 << 20, 1, 1, 512, 513, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));      // beyond YNET_MAP_MODES_MAX_PIXELS
    EXPECT_REJECT(ynet_map_modes(cfp, 1ll << 40, 1, 1, 1 << 20, 1 << 20, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));
    EXPECT_REJECT(ynet_map_modes(cfp, 16, 1ll << 22, 1, 4, 4, 20, 3, 1.f, fp, fp, fp, &status, &status, nullptr));       // too many planes for one grid
    EXPECT_REJECT(ynet_resize_nearest(nullptr, (int*)dummy, 4, 4, 2, 2, 0.5, 0.5, nullptr));
    EXPECT_REJECT(ynet_resize_nearest((const int*)dummy, (int*)dummy, 4, 4, 2, 2, 0.0, 0.5, nullptr));      // factor 0
    EXPECT_REJECT(ynet_upconv_dgrad_ring(nullptr, 0, cfp, nullptr, 0, fp, 0, 1, 64, 32, 8, 8, nullptr));
    EXPECT_REJECT(ynet_upconv_dgrad_ring(cfp, 64 * 64, cfp, nullptr, 0, fp, 32 * 64, 1, 62, 32, 8, 8, nullptr));        // C4 not a multiple of 4
    EXPECT_REJECT(ynet_upconv_dgrad_ring(cfp, 8, cfp, nullptr, 0, fp, 32 * 64, 1, 64, 32, 8, 8, nullptr));               // batch stride below the image
    EXPECT_REJECT(ynet_upconv_dgrad_ring(cfp, 512 * 64, cfp, nullptr, 0, fp, 64 * 64, 1, 512, 64, 8, 8, nullptr));       // tables beyond 64 KB of LDS
    EXPECT_REJECT(ynet_conv2d_winograd_s2d(nullptr, 0, cfp, fp, 0, 32, 16, 8, 256, 256, nullptr));
    EXPECT_REJECT(ynet_conv2d_winograd_s2d(cfp, 32ll * 64 * 64, cfp, fp, 16ll * 64 * 64, 32, 16, 1, 64, 64, nullptr));   // too few pixels for the Winograd kernels
    // the [16, 32]-channel data gradient in one launch and the last decoder convolution inside the predictor + criterion (round 6)
    if (ynet_conv2d_winograd_split_supported(8, 256, 256, 32) != 1 || ynet_conv2d_winograd_split_supported(8, 256, 256, 16) != 0) ++failures;
    EXPECT_REJECT(ynet_conv2d_winograd_split(nullptr, 0, cfp, fp, 0, 0, fp, 0, 32, 8, 256, 256, nullptr));
    EXPECT_REJECT(ynet_conv2d_winograd_split(cfp, 32ll * 65536, cfp, fp, 16ll * 65536, 1, nullptr, 0, 32, 8, 256, 256, nullptr));      // no second destination
    EXPECT_REJECT(ynet_conv2d_winograd_split(cfp, 32ll * 65536, cfp, fp, 16ll * 65536, 0, fp, 8, 32, 8, 256, 256, nullptr));            // its batch stride below the image
    if (ynet_conv2d_winograd_pred_bce_supported(32, 256, 256, 32, 32, 12, 31) != 1 || ynet_conv2d_winograd_pred_bce_supported(16, 512, 512, 32, 32, 30, 31) != 1 || ynet_conv2d_winograd_pred_bce_supported(32, 256, 256, 32, 32, 33, 31) != 0 ||
        ynet_conv2d_winograd_pred_bce_supported(512, 256, 256, 32, 32, 12, 31) != 0 || ynet_conv2d_winograd_pred_bce_supported(8, 256, 256, 16, 32, 12, 31) != 0)
        ++failures;      // (<= 32 predictor outputs, tables within LDS, 32 -> 32)
    EXPECT_REJECT(ynet_conv2d_winograd_pred_bce_blob(nullptr, 0, cfp, cfp, cfp, cfp, 12, cfp, cfp, 31, 400, fp, fp, fp, 0, fp, 8, 256, 256, 1.f, nullptr));
    EXPECT_REJECT(ynet_conv2d_winograd_pred_bce_blob(cfp, 32ll * 65536, cfp, cfp, cfp, cfp, 33, cfp, cfp, 31, 400, fp, fp, fp, 32ll * 65536, fp, 8, 256, 256, 1.f, nullptr));   // 33 outputs
    EXPECT_REJECT(ynet_conv2d_winograd_pred_bce_blob(cfp, 32ll * 65536, cfp, cfp, cfp, cfp, 12, cfp, cfp, 31, 128, fp, fp, fp, 32ll * 65536, fp, 8, 256, 256, 1.f, nullptr));   // template smaller than the window
    EXPECT_REJECT(ynet_batchnorm2d_fwd(nullptr, fp, nullptr, nullptr, nullptr, nullptr, fp, fp, nullptr, 1, 4, 16, 1, 0.1, 1e-5, nullptr));
    EXPECT_REJECT(ynet_batchnorm2d_fwd(cfp, fp, nullptr, nullptr, nullptr, nullptr, fp, fp, nullptr, 1, 4, 16, 1, 0.1, 1e-5, nullptr));      // training mode without a workspace
    EXPECT_REJECT(ynet_batchnorm2d_fwd(cfp, fp, nullptr, nullptr, nullptr, nullptr, fp, fp, nullptr, 1, 4, 16, 0, 0.1, 1e-5, nullptr));      // evaluation mode without running statistics
    EXPECT_REJECT(ynet_batchnorm2d_bwd(cfp, cfp, cfp, cfp, nullptr, fp, nullptr, nullptr, nullptr, 1, 4, 16, 1, nullptr));
    EXPECT_REJECT(ynet_add_relu(nullptr, cfp, fp, 4, 1, nullptr));
    EXPECT_REJECT(ynet_relu_bwd(cfp, cfp, nullptr, 4, nullptr));
    if (ynet_batchnorm_workspace_doubles(16) != 2ll * 16 * 64 || ynet_batchnorm_workspace_doubles(0) != 0) { fprintf(stderr, "batchnorm workspace\n"); ++failures; }
    EXPECT_REJECT(ynet_rot90_flip(nullptr, dummy, 1, 4, 4, 1, 0, nullptr));
    EXPECT_REJECT(ynet_rot90_flip(dummy, dummy, 1, 4, 4, 1, 0, nullptr));      // in place
    EXPECT_REJECT(ynet_rot_coords(nullptr, 4, 0, 0, 1, 0, 0, 1, 0, 0, nullptr));
    {   // ynet_conv2d_auto: the host half -- descriptor checks, the plan, the cache size -- without a launch
        EXPECT_REJECT(ynet_conv2d_auto(nullptr, nullptr, nullptr));
        YnetConvAuto d;
        memset(&d, 0, sizeof(d));
        EXPECT_REJECT(ynet_conv2d_auto(&d, nullptr, nullptr));                   // no sources / filter
        d.nsrc = 1; d.ndst = 1; d.src[0] = cfp; d.src_c[0] = 32; d.src_bs[0] = 32ll * 256 * 256; d.wp = cfp;
        d.dst[0] = fp; d.dst_c[0] = 32; d.dst_bs[0] = 32ll * 256 * 256; d.B = 8; d.H = 256; d.W = 256; d.K = 3; d.relu = 1;
        const long long need = ynet_conv2d_auto_cache_floats(&d);
        if (need != ynet_winograd_filter_floats(32, 32)) { fprintf(stderr, "conv2d_auto cache floats %lld\n", need); ++failures; }
        long long lf = 0;
        if (ynet_conv2d_auto_cache_layout(&d, &lf) == 0 || lf != need) { fprintf(stderr, "conv2d_auto cache layout: %lld floats\n", lf); ++failures; }
        EXPECT_REJECT(ynet_conv2d_auto(&d, nullptr, nullptr));                   // a Winograd plan without a cache
        d.flags = YNET_AUTO_NO_WINOGRAD;
        if (ynet_conv2d_auto_cache_floats(&d) != 0) { fprintf(stderr, "conv2d_auto: implicit GEMM needs no cache\n"); ++failures; }
        d.flags = 0; d.K = 4;
        EXPECT_REJECT(ynet_conv2d_auto(&d, nullptr, nullptr));                   // K
        d.K = 3; d.upsample2x = 1; d.src_c[0] = 8; d.H = 32; d.W = 32;
        EXPECT_REJECT(ynet_conv2d_auto(&d, nullptr, nullptr));                   // no up-convolution kernel serves 8 channels at 32^2
        d.upsample2x = 0; d.H = 256; d.W = 256; d.src_c[0] = 32; d.addend = cfp; d.pooled = fp;
        EXPECT_REJECT(ynet_conv2d_auto(&d, nullptr, nullptr));                   // addend + pooled
        d.addend = nullptr; d.dst_c[0] = 64; d.dst_bs[0] = 64ll * 256 * 256; d.pooled = nullptr;
        if (ynet_conv2d_auto_cache_floats(&d) <= 0) { fprintf(stderr, "conv2d_auto: 32 -> 64 at 256^2 is a Winograd plan\n"); ++failures; }
        if (ynet_conv2d_auto_workspace_floats(&d) != 0) { fprintf(stderr, "conv2d_auto: no workspace for a large map\n"); ++failures; }
    }
    void* comm = nullptr;
    EXPECT_REJECT(ynet_comm_create(3, 2, 16, &comm));
    EXPECT_REJECT(ynet_comm_create(0, 99, 16, &comm));
    EXPECT_REJECT(ynet_comm_export(nullptr, dummy));
    EXPECT_REJECT(ynet_comm_connect(nullptr, dummy));
    EXPECT_REJECT(ynet_allreduce_sum(nullptr, fp, 4, nullptr));
    if (ynet_comm_destroy(nullptr) != 0) ++failures;
    printf("asan host driver: %d failures, checksum %lld\n", failures, acc);
    return failures ? 1 : 0;
}
