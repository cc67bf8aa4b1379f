// The 3-D ResNet-18 training trunk as one object, host side only: the plan of its convs and blocks, the binding of its parameters and
// gradients, the layout of `saved` and of the workspace, and the forward and backward walks over the stem, the pool and the eight blocks.
// The temporal discriminator (i2v_disc3d.hip) and the motion encoder's training path (i2v_encoder_train.hip) each embed one R3Trunk and
// add their head; the kernels and their launchers are in i2v_res3d_trunk.h.  Included into the anonymous namespace of its users.
#pragma once
#include "i2v_res3d_trunk.h"

#include <string>

namespace i2v {
namespace {

struct R3Block { int c1, c2, cd, in; };   // conv indices (cd -1: no downsample branch); in: the conv whose activation enters (-1: the pool's output)

struct R3Trunk {
    int nconv = 0, pool = 0;
    TcConv L[D3_MAXCONV];
    std::string wkey[D3_MAXCONV], nkey[D3_MAXCONV];   // state-dict prefixes of the conv and of its GroupNorm
    R3Block B[8];
    float *w[D3_MAXCONV] = {}, *u[D3_MAXCONV] = {}, *v[D3_MAXCONV] = {}, *nw[D3_MAXCONV] = {}, *nb[D3_MAXCONV] = {};
    float *gw[D3_MAXCONV] = {}, *gnw[D3_MAXCONV] = {}, *gnb[D3_MAXCONV] = {};
    int last() const { return B[7].c2; }   // the conv whose activation the head takes
};

// What the two networks' plans differ in
struct R3Rules {
    int stem_st, stem_ss;          // the stem's strides
    int sn_block0, sn_down;        // spectral norm on conv1 / conv2 of block 0 of a layer, and on its downsample conv
    int pool;                      // MaxPool3d behind the stem
    bool downsample_on_stride_t;   // the downsample rule has the stride_t term
};

void r3_build(R3Trunk& k, const int32_t* channels, const int32_t* stride_s, const int32_t* stride_t, const R3Rules& r) {
    k.pool = r.pool;
    int n = 0;
    auto add = [&](const TcConv& c, const std::string& conv, const std::string& norm) {
        k.L[n] = c; k.wkey[n] = conv; k.nkey[n] = norm;
        return n++;
    };
    add(make_conv(3, channels[0], true, r.stem_st, r.stem_ss, 0), "conv1", "norm1");
    int inplanes = channels[0], prev = k.pool ? -1 : 0;
    for (int l = 0; l < 4; ++l) {
        const int planes = channels[l + 1], ss = stride_s[l], st = stride_t[l];
        const std::string p0 = "layer." + std::to_string(l) + ".0.", p1 = "layer." + std::to_string(l) + ".1.";
        R3Block b0{}, b1{};
        b0.in = prev;
        b0.c1 = add(make_conv(inplanes, planes, false, st, ss, r.sn_block0), p0 + "conv1", p0 + "bn1");
        b0.c2 = add(make_conv(planes, planes, false, 1, 1, r.sn_block0), p0 + "conv2", p0 + "bn2");
        b0.cd = -1;
        // resnet3D.py:265: the discriminator's rule has the stride_t term; resnet3D.py:184: the encoder's has none
        if (ss != 1 || inplanes != planes || (r.downsample_on_stride_t && st != 1))
            b0.cd = add(make_conv(inplanes, planes, false, st, ss, r.sn_down), p0 + "downsample.0", p0 + "downsample.1");
        b1.in = b0.c2;
        b1.c1 = add(make_conv(planes, planes, false, 1, 1, 0), p1 + "conv1", p1 + "bn1");
        b1.c2 = add(make_conv(planes, planes, false, 1, 1, 0), p1 + "conv2", p1 + "bn2");
        b1.cd = -1;
        k.B[2 * l] = b0; k.B[2 * l + 1] = b1;
        prev = b1.c2;
        inplanes = planes;
    }
    k.nconv = n;
}

bool bound_ptr(const StateDict& s, const std::string& key, int64_t numel, float** out) {
    const float* p = s.f32(key, numel);
    *out = const_cast<float*>(p);
    return p != nullptr;
}

// the trunk's keys; the callers bind their head's afterwards
int r3_bind(R3Trunk& k, const StateDict& sd) {
    for (int i = 0; i < k.nconv; ++i) {
        const TcConv& c = k.L[i];
        const int64_t wn = (int64_t)c.cout * c.cin * ntap_of(c);
        if (!bound_ptr(sd, k.wkey[i] + (c.sn ? ".weight_orig" : ".weight"), wn, &k.w[i])) return I2V_E_MISSING;
        if (c.sn && (!bound_ptr(sd, k.wkey[i] + ".weight_u", c.cout, &k.u[i]) || !bound_ptr(sd, k.wkey[i] + ".weight_v", wn / c.cout, &k.v[i])))
            return I2V_E_MISSING;
        if (!bound_ptr(sd, k.nkey[i] + ".weight", c.cout, &k.nw[i]) || !bound_ptr(sd, k.nkey[i] + ".bias", c.cout, &k.nb[i])) return I2V_E_MISSING;
    }
    return I2V_OK;
}

int r3_bind_grads(R3Trunk& k, const StateDict& gd) {
    for (int i = 0; i < k.nconv; ++i) {
        const TcConv& c = k.L[i];
        if (!bound_ptr(gd, k.wkey[i] + (c.sn ? ".weight_orig" : ".weight"), (int64_t)c.cout * c.cin * ntap_of(c), &k.gw[i])) return I2V_E_MISSING;
        if (!bound_ptr(gd, k.nkey[i] + ".weight", c.cout, &k.gnw[i]) || !bound_ptr(gd, k.nkey[i] + ".bias", c.cout, &k.gnb[i])) return I2V_E_MISSING;
    }
    return I2V_OK;
}

// What a network adds behind the trunk: the words that end the refusal ("... not on the [1, 4, 4] that <head>"), up to three entries
// at the end of `saved` (bytes; 0: none) and one at the end of the workspace
struct R3Extra { const char* head; size_t saved[3]; size_t ws; };

// Where everything lies for one input shape: `saved` (offsets from its base) and the workspace
struct R3Layout {
    bool ok = false;
    char why[160] = "";
    int n = 0;
    TcGeo geo[D3_MAXCONV];
    int pt = 0, ph = 0, pw = 0, pho = 0, pwo = 0;   // the pool's input and output map
    long pool_in = 0, pool_out = 0;                 // positions
    size_t x4 = 0, pre[D3_MAXCONV] = {}, act[D3_MAXCONV] = {}, stats[D3_MAXCONV] = {}, wf[D3_MAXCONV] = {}, wd[D3_MAXCONV] = {}, sigma[D3_MAXCONV] = {},
           us[D3_MAXCONV] = {}, vs[D3_MAXCONV] = {}, pout = 0, parg = 0, tail[3] = {}, saved_total = 0;
    size_t pi_t[D3_MAXCONV] = {}, pi_s[D3_MAXCONV] = {}, fwd = 0, gbuf[4] = {}, dc[2] = {}, part = 0, dwn = 0, dotp = 0, gn = 0, ws_tail = 0, ws_total = 0;
};

R3Layout r3_layout(const R3Trunk& d, int n, int t, int h, int w, const R3Extra& extra) {
    R3Layout y;
    if (n <= 0 || t <= 0 || h <= 0 || w <= 0) {
        snprintf(y.why, sizeof y.why, "batch %d, clip %d x %d x %d", n, t, h, w);
        return y;
    }
    y.n = n;
    // the maps, conv by conv
    y.geo[0] = make_geo(n, t, h, w, d.L[0]);
    int ct = y.geo[0].to, chh = y.geo[0].ho, cw = y.geo[0].wo;
    if (d.pool && ct > 0 && chh > 0 && cw > 0) {
        y.pt = ct; y.ph = chh; y.pw = cw; y.pho = (chh - 1) / 2 + 1; y.pwo = (cw - 1) / 2 + 1;
        y.pool_in = (long)n * ct * chh * cw; y.pool_out = (long)n * ct * y.pho * y.pwo;
        chh = y.pho; cw = y.pwo;
    }
    for (int b = 0; b < 8; ++b) {
        const R3Block& k = d.B[b];
        if (ct < 1 || chh < 1 || cw < 1) break;
        y.geo[k.c1] = make_geo(n, ct, chh, cw, d.L[k.c1]);
        if (k.cd >= 0) y.geo[k.cd] = make_geo(n, ct, chh, cw, d.L[k.cd]);
        ct = y.geo[k.c1].to; chh = y.geo[k.c1].ho; cw = y.geo[k.c1].wo;
        y.geo[k.c2] = make_geo(n, ct, chh, cw, d.L[k.c2]);
    }
    if (ct != 1 || chh != 4 || cw != 4) {
        snprintf(y.why, sizeof y.why, "a clip of %d frames of %d x %d ends on a [%d, %d, %d] map, not on the [1, 4, 4] that %s", t, h, w, ct, chh, cw,
                 extra.head);
        return y;
    }
    Carver s;
    y.x4 = s.take_floats((size_t)y.geo[0].mi * 4);
    size_t gmax = 0, pmax = 0, emax = 0, bmax = 0, cmax = 0;
    for (int i = 0; i < d.nconv; ++i) {
        const TcConv& c = d.L[i];
        const size_t elems = (size_t)y.geo[i].mo * c.cout;
        y.pre[i] = s.take_floats(elems);
        y.act[i] = s.take_floats(elems);
        y.stats[i] = s.take_bytes((size_t)n * D3_GROUPS * 2 * 8);
        y.wf[i] = s.take_floats((size_t)ntap_of(c) * c.cout * c.cinp);
        y.wd[i] = s.take_floats(pack_elems(c));
        y.sigma[i] = s.take_floats(c.sn ? 1 : 0);
        y.us[i] = s.take_floats(c.sn ? c.cout : 0);
        y.vs[i] = s.take_floats(c.sn ? (size_t)c.cin * ntap_of(c) : 0);
        gmax = std::max(gmax, std::max(elems, (size_t)y.geo[i].mi * c.cinp));
        pmax = std::max(pmax, wgrad_part_floats(c, y.geo[i].mo));
        emax = std::max(emax, (size_t)c.cout * c.cin * ntap_of(c));
        bmax = std::max(bmax, finish_blocks(c));
        cmax = std::max(cmax, (size_t)c.cout);
    }
    if (d.pool) {
        y.pout = s.take_floats((size_t)y.pool_out * d.L[0].cout);
        y.parg = s.take_floats((size_t)y.pool_out * d.L[0].cout);
    }
    for (int i = 0; i < 3; ++i) y.tail[i] = s.take_bytes(extra.saved[i]);
    y.saved_total = s.total();
    Carver k;
    for (int i = 0; i < d.nconv; ++i) {
        y.pi_t[i] = k.take_bytes(d.L[i].sn ? (size_t)d.L[i].cin * ntap_of(d.L[i]) * 8 : 0);
        y.pi_s[i] = k.take_bytes(d.L[i].sn ? (size_t)d.L[i].cout * 8 : 0);
    }
    y.fwd = k.take_bytes(y.saved_total);
    for (int i = 0; i < 4; ++i) y.gbuf[i] = k.take_floats(gmax);
    for (int i = 0; i < 2; ++i) y.dc[i] = k.take_floats(gmax);
    y.part = k.take_floats(pmax);
    y.dwn = k.take_floats(emax);
    y.dotp = k.take_bytes((bmax + 1) * 8);
    y.gn = k.take_bytes(gn_ws(n, (int)cmax).total);
    y.ws_tail = k.take_bytes(extra.ws);
    y.ws_total = k.total();
    y.ok = true;
    return y;
}

int r3_refuse(const char* what, const R3Layout& y) {
    set_error("%s: %s", what, y.why);
    return I2V_E_INVALID;
}

// the per-conv entries of a saved_layout table; the caller appends its own with put()
struct R3Table {
    int32_t *kind, *conv, *dims;
    int64_t* offset;
    int count = 0;
    void put(int kd, int ci, int mt, int mh, int mw, int mc, size_t off) {
        const int e = count++;
        kind[e] = kd; conv[e] = ci; dims[4 * e] = mt; dims[4 * e + 1] = mh; dims[4 * e + 2] = mw; dims[4 * e + 3] = mc; offset[e] = (int64_t)off;
    }
    void put_convs(const R3Trunk& d, const R3Layout& y, int kind_pre, int kind_act) {
        for (int i = 0; i < d.nconv; ++i) {
            put(kind_pre, i, y.geo[i].to, y.geo[i].ho, y.geo[i].wo, d.L[i].cout, y.pre[i]);
            put(kind_act, i, y.geo[i].to, y.geo[i].ho, y.geo[i].wo, d.L[i].cout, y.act[i]);
        }
    }
};

// x [N][3][T][H][W] -> every map of `sv`; the last activation is left at y.act[d.last()] of `sv`.  `iterate`: the spectral-normed convs
// do a power iteration (none is launched where no conv is spectral-normed); fmaps: null, or four pointers (null: not wanted) that
// receive the activation behind each layer.
int r3_forward(const R3Trunk& d, const R3Layout& y, const float* x, bool iterate, float* const* fmaps, void* sv, void* workspace, hipStream_t st) {
    void* gnws = Carver::at<char>(workspace, y.gn);
    const int nc = d.nconv, n = y.n;

    float* x4 = Carver::at(sv, y.x4);
    hipLaunchKernelGGL(tc_input4_kernel, dim3(grid_for(y.geo[0].mi)), dim3(256), 0, st, x, x4, y.geo[0].mi, y.geo[0].mi / n);
    I2V_LAUNCHED();

    // spectral norm, PD_MAXCONV convs per group of launches
    PdPiArgs pi{};
    pi.iterate = iterate ? 1 : 0;
    for (int i = 0; i < nc; ++i) {
        const TcConv& c = d.L[i];
        if (c.sn) {
            const int cols = c.cin * ntap_of(c);
            pi.c[pi.nconv++] = PdPiConv{d.w[i], d.u[i], d.v[i], Carver::at(sv, y.sigma[i]), Carver::at(sv, y.us[i]), Carver::at(sv, y.vs[i]),
                                        Carver::at<double>(workspace, y.pi_t[i]), Carver::at<double>(workspace, y.pi_s[i]), c.cout, cols, pi.btotal, pi.rtotal};
            pi.btotal += (cols + 63) / 64; pi.rtotal += c.cout;
        }
        if (pi.nconv == PD_MAXCONV || (i + 1 == nc && pi.nconv > 0)) {
            if (int rc = launch_power_iteration(pi, st)) return rc;
            pi.nconv = pi.btotal = pi.rtotal = 0;
        }
    }
    TcPackArgs pk{};
    pk.nconv = nc;
    for (int i = 0; i < nc; ++i) {
        const TcConv& c = d.L[i];
        pk.c[i] = TcPackConv{d.w[i], c.sn ? Carver::at(sv, y.sigma[i]) : nullptr, Carver::at(sv, y.wf[i]), Carver::at(sv, y.wd[i]),
                             c.cout, c.cin, c.cinp, c.cind, ntap_of(c), pk.total};
        pk.total += (long)pack_elems(c);
    }
    if (int rc = launch_pack<Trunk3d>(pk, st)) return rc;

    // conv i on `in`, then its GroupNorm (+ res) (ReLU) -> act[i]
    auto conv_gn = [&](int i, const float* in, const float* res, bool relu) -> int {
        const TcConv& c = d.L[i];
        float* pre = Carver::at(sv, y.pre[i]);
        if (int rc = launch_conv<Trunk3d>(c, in, Carver::at(sv, y.wf[i]), pre, y.geo[i], st)) return rc;
        return launch_gn(pre, res, d.nw[i], d.nb[i], n, y.geo[i].mo / n, c.cout, relu, Carver::at(sv, y.act[i]), Carver::at<double>(sv, y.stats[i]),
                         gnws, st);
    };
    if (int rc = conv_gn(0, x4, nullptr, true)) return rc;
    if (d.pool) {
        const long total = y.pool_out * d.L[0].cout;
        hipLaunchKernelGGL(d3_maxpool_kernel, dim3(grid_for(total)), dim3(256), 0, st, Carver::at(sv, y.act[0]), Carver::at(sv, y.pout),
                           Carver::at<int>(sv, y.parg), total, y.pt, y.ph, y.pw, y.pho, y.pwo, d.L[0].cout);
        I2V_LAUNCHED();
    }
    for (int b = 0; b < 8; ++b) {
        const R3Block& k = d.B[b];
        const float* in = k.in < 0 ? Carver::at(sv, y.pout) : Carver::at(sv, y.act[k.in]);
        if (int rc = conv_gn(k.c1, in, nullptr, true)) return rc;
        const float* res = in;
        if (k.cd >= 0) {
            if (int rc = conv_gn(k.cd, in, nullptr, false)) return rc;
            res = Carver::at(sv, y.act[k.cd]);
        }
        if (int rc = conv_gn(k.c2, Carver::at(sv, y.act[k.c1]), res, true)) return rc;
        if ((b & 1) && fmaps && fmaps[b / 2])
            I2V_HIP_CHECK(hipMemcpyAsync(fmaps[b / 2], Carver::at(sv, y.act[k.c2]), (size_t)y.geo[k.c2].mo * d.L[k.c2].cout * 4, hipMemcpyDeviceToDevice, st));
    }
    return I2V_OK;
}

// The caller's head has written the gradient at the last activation into gbuf[0] of the workspace.  d_fmaps: null, or four gradients
// (null: none) at the activations behind the layers, added where the walk reaches them.  The parameter gradients (`pg`) go to the bound
// tensors, written or (`acc`) added; d_x (null: not wanted) receives the frames' gradient.
int r3_backward(const R3Trunk& d, const R3Layout& y, const float* const* d_fmaps, void* sv, float* d_x, bool pg, bool acc, void* workspace,
                hipStream_t st) {
    const int n = y.n;
    float* part = Carver::at(workspace, y.part);
    float* dwn = Carver::at(workspace, y.dwn);
    double* dotp = Carver::at<double>(workspace, y.dotp);
    void* gnws = Carver::at<char>(workspace, y.gn);
    float* G = Carver::at(workspace, y.gbuf[0]);      // the gradient at the current block's output
    float* Gn = Carver::at(workspace, y.gbuf[1]);     // ... at its input
    float* H1 = Carver::at(workspace, y.gbuf[2]);     // ... at conv1's activation
    float* X2 = Carver::at(workspace, y.gbuf[3]);     // the downsample branch's share of Gn
    float* DC = Carver::at(workspace, y.dc[0]);       // ... at a conv's output
    float* DC2 = Carver::at(workspace, y.dc[1]);

    // GroupNorm of conv i backwards: g (masked by `mask`) -> dc; then the conv's weight gradient
    auto norm_conv_bwd = [&](int i, const float* g, const float* mask, const float* xin, float* dc) -> int {
        const TcConv& c = d.L[i];
        if (int rc = launch_gn_bwd(g, mask, Carver::at(sv, y.pre[i]), Carver::at<double>(sv, y.stats[i]), d.nw[i], n, y.geo[i].mo / n, c.cout, dc,
                                   pg ? d.gnw[i] : nullptr, pg ? d.gnb[i] : nullptr, acc, gnws, st))
            return rc;
        if (!pg) return I2V_OK;
        return launch_wgrad<Trunk3d>(c, dc, nullptr, nullptr, xin, d.w[i], c.sn ? Carver::at(sv, y.us[i]) : nullptr, c.sn ? Carver::at(sv, y.vs[i]) : nullptr,
                            c.sn ? Carver::at(sv, y.sigma[i]) : nullptr, part, dwn, dotp, d.gw[i], acc, y.geo[i], st);
    };
    for (int b = 7; b >= 0; --b) {
        const R3Block& k = d.B[b];
        if ((b & 1) && d_fmaps && d_fmaps[b / 2]) {   // G is at the activation behind layer b / 2
            const long elems = y.geo[k.c2].mo * d.L[k.c2].cout;
            hipLaunchKernelGGL(d3_add_kernel, dim3(grid_for(elems)), dim3(256), 0, st, G, d_fmaps[b / 2], elems);
            I2V_LAUNCHED();
        }
        const float* out = Carver::at(sv, y.act[k.c2]);
        const float* xin = k.in < 0 ? Carver::at(sv, y.pout) : Carver::at(sv, y.act[k.in]);
        const float* h1 = Carver::at(sv, y.act[k.c1]);
        if (int rc = norm_conv_bwd(k.c2, G, out, h1, DC)) return rc;
        if (int rc = launch_dgrad<Trunk3d>(d.L[k.c2], DC, nullptr, nullptr, Carver::at(sv, y.wd[k.c2]), nullptr, nullptr, H1, false, n, y.geo[k.c2], st)) return rc;
        if (int rc = norm_conv_bwd(k.c1, H1, h1, xin, DC)) return rc;
        if (k.cd >= 0) {
            if (int rc = norm_conv_bwd(k.cd, G, out, xin, DC2)) return rc;
            if (int rc = launch_dgrad<Trunk3d>(d.L[k.cd], DC2, nullptr, nullptr, Carver::at(sv, y.wd[k.cd]), nullptr, nullptr, X2, false, n, y.geo[k.cd], st)) return rc;
            if (int rc = launch_dgrad<Trunk3d>(d.L[k.c1], DC, nullptr, nullptr, Carver::at(sv, y.wd[k.c1]), X2, nullptr, Gn, false, n, y.geo[k.c1], st)) return rc;
        } else if (int rc = launch_dgrad<Trunk3d>(d.L[k.c1], DC, nullptr, nullptr, Carver::at(sv, y.wd[k.c1]), G, out, Gn, false, n, y.geo[k.c1], st)) {
            return rc;
        }
        std::swap(G, Gn);
    }
    // G: the gradient at the pool's output (or at the stem's activation)
    if (d.pool) {
        const long total = y.pool_in * d.L[0].cout;
        hipLaunchKernelGGL(d3_maxpool_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, st, G, Carver::at<int>(sv, y.parg), Gn, total, y.pt, y.ph, y.pw,
                           y.pho, y.pwo, d.L[0].cout);
        I2V_LAUNCHED();
        std::swap(G, Gn);
    }
    if (int rc = norm_conv_bwd(0, G, Carver::at(sv, y.act[0]), Carver::at(sv, y.x4), DC)) return rc;
    if (d_x)
        if (int rc = launch_dgrad<Trunk3d>(d.L[0], DC, nullptr, nullptr, Carver::at(sv, y.wd[0]), nullptr, nullptr, d_x, true, n, y.geo[0], st)) return rc;
    return I2V_OK;
}

}  // namespace
}  // namespace i2v
