"""An independent float64 restatement (numpy) of the rlGgx closure and NDProfile, written from the reference's lines -- NOT
from oracle/rls_oracle.c -- as a second anchor for the oracle: a transcription error would have to be made twice, in two
languages, to go unnoticed.  Each function cites the lines it follows.  The twin evaluates every formula in float64 from the
float32 inputs, with the reference's branch structure; two quantities are formed in float32 as the reference forms them,
because their fp32 value IS the value the reference's branches and results depend on: the rational fit of the second slope
(its denominator cancels to 4.9e-4 at u = 1) and the comparisons against AI_EPSILON thresholds.

Beyond one sample -- the loops and rlSkin's layering, over the numbers of oracle_lib.batch_sample_02 (the project's stand-in
for the closed AiSampler; sample streams as oracle/rls_oracle.h and include/rlshaders_amd.h name them):
  Ggx64.integrate            the loop over evalSample / evalBrdf / evalPdf, the Fresnel mean        src/rlGgx.h:97-127, 172-184
  Ggx64.refract, .integrate_refract   the traced loop (mirror on TIR) and the untraced refraction   src/rlGgx.h:205-245
  Disney64.integrate         the explicit loop of both lobes: validity, sums of f / pdf, counts     src/rlDisney.cpp:299-312
  Sss64                      frame 143-167, mis_pdf 252-263, cavity_fade 401-413, integrate_scatter 227-276 with the walk of
                             288-357 and the shading of 379-424 over the analytic plane / sphere    src/rlSss.h
  skin64, skin_integrate64   the layer arithmetic with one sample / n^2 samples per lobe            src/rlSkin.cpp:174-254
The closed services stay the project's stand-ins on both sides (Snell's law for AiRefractRay, the mirror for AiReflectRay, a
uniform environment for AiTrace, one distant Lambertian light, ray/plane and ray/sphere intersections, here in float64).
Test infrastructure only (tests/test_oracle_float64_twin.py, tests/twin_loops_util.py, tools/studies/)."""
import numpy as np

F = np.float32
EPS = float(F(1e-4))


def _norm(v):
    n = np.linalg.norm(v, axis=0)
    return v / np.where(n > 0, n, 1.0)


class Ggx64:
    """GgxSamplerT's constructor, src/rlGgx.h:130-156: iors, frame (U = tangent, V = N x U), alphas, mRoughness"""

    def __init__(self, c):
        self.wo, self.N, self.T = (np.asarray(c[k], np.float64) for k in ("wo", "N", "T"))
        n = self.wo.shape[1]
        full = lambda v: np.broadcast_to(np.asarray(v, np.float64), (n,))
        rough, aniso, ior = full(c["roughness"]), full(c["anisotropic"]), full(c["ior"])
        ks = np.asarray(c["KsColor"], np.float64)
        self.ks = ks if ks.ndim == 2 else np.repeat(ks[:, None], n, axis=1)
        self.iorIn, self.iorOut = np.ones(n), np.maximum(ior, 1e-4)
        if c.get("exiting") is not None:                                    # isEntering false: the iors swap, 137-142
            ex = np.broadcast_to(np.asarray(c["exiting"]).astype(bool), (n,))
            self.iorIn, self.iorOut = np.where(ex, self.iorOut, self.iorIn), np.where(ex, self.iorIn, self.iorOut)
        self.U, self.V = self.T, np.cross(self.N.T, self.T.T).T
        aspect = np.sqrt(1.0 - aniso * 0.9)
        self.ax = np.maximum(1e-4, rough * rough / aspect)
        self.ay = np.maximum(1e-4, rough * rough * aspect)
        self.rough = np.maximum(1e-5, rough * rough)

    # src/rlGgx.cpp:14-61
    def _slope(self, theta, rx, ry, ry32):
        with np.errstate(all="ignore"):
            r = np.sqrt(rx / (1.0 - rx))
            ux, uy = r * np.cos(2 * np.pi * ry), r * np.sin(2 * np.pi * ry)
            B = np.tan(theta)
            B2 = B * B
            G1 = 2.0 / (1.0 + np.sqrt(1.0 + B2))
            A = 2.0 * rx / G1 - 1.0
            A2 = A * A
            tmp = 1.0 / (A2 - 1.0)
            D = np.sqrt(np.maximum(0.0, B2 * tmp * tmp - (A2 - B2) * tmp))
            x1, x2 = B * tmp - D, B * tmp + D
            sx = np.where((A < 0) | (x2 > 1.0 / B), x1, x2)
            up = ry32 > F(0.5)
            u = np.where(up, (F(2) * (ry32 - F(0.5)).astype(F)).astype(F), (F(2) * (F(0.5) - ry32).astype(F)).astype(F)).astype(F)
            m = lambda a, b: (a * b).astype(F)
            num = m(u, (m(u, (m(u, F(0.27385)) - F(0.73369)).astype(F)) + F(0.46341)).astype(F))
            den = (m(u, (m(u, (m(u, F(0.093073)) + F(0.309420)).astype(F)) - F(1.0)).astype(F)) + F(0.597999)).astype(F)
            z = num.astype(np.float64) / den.astype(np.float64)
            sy = np.where(up, 1.0, -1.0) * z * np.sqrt(1.0 + sx * sx)
            uniform = (theta < EPS) | (np.abs(A2 - 1.0) < EPS)
        return np.where(uniform, ux, sx), np.where(uniform, uy, sy)

    # VNDFKernel::evalSample, src/rlGgx.cpp:63-99
    def microfacet(self, rx32, ry32):
        rx, ry = rx32.astype(np.float64), ry32.astype(np.float64)
        V = self.wo
        cosv = np.clip((self.N * V).sum(0), -1.0, 1.0)
        phiv = np.arctan2((self.V * V).sum(0), (self.U * V).sum(0))
        sinv = np.sqrt(np.maximum(0.0, 1.0 - cosv * cosv))                  # sphericalDirection, src/rlUtil.h:21-29
        l = _norm(np.stack([sinv * np.cos(phiv) * self.ax, sinv * np.sin(phiv) * self.ay, cosv]))
        flat = ~(l[2] < 1.0 - EPS)
        theta = np.where(flat, 0.0, np.arccos(np.clip(l[2], -1, 1)))
        phi = np.where(flat, 0.0, np.arctan2(l[1], l[0]))
        sx, sy = self._slope(theta, rx, ry, ry32)
        c, s = np.cos(phi), np.sin(phi)
        ox, oy = -(c * sx - s * sy) * self.ax, -(s * sx + c * sy) * self.ay
        return _norm(ox * self.U + oy * self.V + self.N)

    # rlUtil reflectDirection, src/rlUtil.h:31-34
    def reflect(self, m):
        return m * (2.0 * np.abs((self.wo * m).sum(0))) - self.wo

    # src/rlGgx.h:249-270
    def fresnel(self, i, m):
        c = np.abs((i * m).sum(0))
        g2 = (self.iorOut / self.iorIn) ** 2 - 1.0 + c * c
        with np.errstate(all="ignore"):
            g = np.sqrt(np.maximum(g2, 0.0))
            gmc, gpc = g - c, g + c
            f = 0.5 * (gmc / gpc) ** 2 * (1.0 + ((c * gpc - 1.0) / (c * gmc + 1.0)) ** 2)
        return np.where(g2 < 0, 1.0, f)

    # src/rlGgx.h:332-340
    def D(self, m):
        mu, mv, mn = (m * self.U).sum(0), (m * self.V).sum(0), (m * self.N).sum(0)
        return (1.0 / np.pi) / (self.ax * self.ay * ((mu / self.ax) ** 2 + (mv / self.ay) ** 2 + mn * mn) ** 2)

    # src/rlGgx.h:343-357
    def G1(self, v, m):
        vm, vn = (v * m).sum(0), (v * self.N).sum(0)
        with np.errstate(all="ignore"):
            g = 2.0 / (1.0 + np.sqrt(1.0 + self.rough ** 2 * (1.0 / (vn * vn) - 1.0)))
        return np.where(vm * vn < 0, 0.0, g)

    # evalPdf, src/rlGgx.h:121-127 with VNDFKernel::evalPdf, 72-80
    def pdf(self, wi):
        H = _norm(self.wo + wi)
        with np.errstate(all="ignore"):
            p = self.D(H) * self.G1(self.wo, H) / np.abs((self.wo * self.N).sum(0)) * 0.25
        return np.maximum(p, EPS)

    # evalBrdf, src/rlGgx.h:110-119, evalReflectance 158-165, reflection 304-313
    def eval(self, wi):
        vn = (self.wo * self.N).sum(0)
        hr = np.where(vn < 0, -1.0, 1.0) * _norm(wi + self.wo)
        ln = (wi * self.N).sum(0)
        with np.errstate(all="ignore"):
            refl = self.fresnel(self.wo, hr) * self.G1(self.wo, hr) * self.G1(wi, hr) * self.D(hr) * 0.25 / (np.abs(ln) * np.abs(vn))
        f = self.ks * (refl * ln)
        small = (np.abs(self.ks) < EPS).all(axis=0) | (wi == 0).all(axis=0)
        return np.where(small, 0.0, f)

    # getSampleWeight, src/rlGgx.h:294-301
    def sample_weight(self, o, m):
        ih = (self.wo * m).sum(0)
        mn, iN = np.abs((m * self.N).sum(0)), np.abs((self.wo * self.N).sum(0))
        with np.errstate(all="ignore"):
            return self.G1(self.wo, m) * self.G1(o, m) * np.abs(ih / (iN * mn))

    def _small_ks(self):
        return (np.abs(self.ks) < EPS).all(axis=0)                          # AiColorIsSmall

    # integrateGlossy's sample loop over the callback triple, src/rlGgx.h:97-127, 172-179 (AiBRDFIntegrate is closed: the
    # sum of evalBrdf / evalPdf is what it accumulates before radiance), with evalSample's Fresnel accumulation (103-104)
    # and getAvgReflectWeight (181-184); a small colour draws no sample at all (174-176), the mean is then 1
    def integrate(self, spp_n, seed, first_index=0, dim_pair=0):
        import oracle_lib as O
        n, spp = self.wo.shape[1], spp_n * spp_n
        total, fres = np.zeros((3, n)), np.zeros(n)
        for s in range(spp):
            rx, ry = O.batch_sample_02(seed, first_index, n, dim_pair, s)
            m = self.microfacet(rx, ry)
            wi = self.reflect(m)
            fres += self.fresnel(wi, m)
            with np.errstate(all="ignore"):
                total += self.eval(wi) / self.pdf(wi)
        small = self._small_ks()
        return np.where(small, 0.0, total), np.where(small, 1.0, fres / spp)

    # the closed AiRefractRay as Snell's law about the normal nrm (the direction leaves on the far side of the surface the
    # view is on); -> (direction, total internal reflection)
    def refract(self, nrm):
        c = (self.wo * nrm).sum(0)
        eta = self.iorIn / self.iorOut
        k = 1.0 + eta * eta * (c * c - 1.0)
        sign = np.where((self.wo * self.N).sum(0) < 0, -1.0, 1.0)
        return (eta * c - sign * np.sqrt(np.maximum(k, 0.0))) * nrm - eta * self.wo, k < 0

    # integrateRefract, src/rlGgx.h:205-245, under a uniform environment env -> (result [3, n], share of TIR samples)
    def integrate_refract(self, spp_n, seed, traced, env, first_index=0, dim_pair=0):
        import oracle_lib as O
        n, spp = self.wo.shape[1], spp_n * spp_n
        env = np.asarray(env, np.float64)[:, None]
        if not traced:                                                      # 212-222
            d, tir = self.refract(self.N)
            w = (self.iorOut / self.iorIn) ** 2 * np.abs((self.N * d).sum(0))
            return env * np.where(tir, 0.0, w), tir.astype(np.float64)
        acc, ntir = np.zeros(n), np.zeros(n)
        for s in range(spp):                                                # 228-243
            rx, ry = O.batch_sample_02(seed, first_index, n, dim_pair, s)
            m = self.microfacet(rx, ry)
            d, tir = self.refract(m)
            d = np.where(tir, m * (2.0 * (self.wo * m).sum(0)) - self.wo, d)    # the closed AiReflectRay: the mirror direction
            acc += self.sample_weight(d, m)
            ntir += tir
        return env * (acc / spp), ntir / spp


class NdProfile64:
    """NDProfile, src/rlSss.h:27-61, src/rlSss.cpp:20-106 (scatter distances already multiplied)"""

    def __init__(self, dist):
        self.d = np.asarray(dist, np.float64)
        self.maxR = self.d.max(axis=0) * 3.0
        with np.errstate(all="ignore"):
            self.c1 = 1.0 - np.exp(-self.maxR / self.d)
            self.c2 = 1.0 - np.exp(-self.maxR / self.d / 3.0)

    def radius(self, rx32):
        rx = rx32.astype(np.float64)
        lo = np.where(rx32 < F(0.3333), 0.0, np.where(rx32 > F(0.6666), float(F(0.6666)), float(F(0.3333))))
        hi = np.where(rx32 < F(0.3333), float(F(0.3333)), np.where(rx32 > F(0.6666), 1.0, float(F(0.6666))))
        k = np.where(rx32 < F(0.3333), 0, np.where(rx32 > F(0.6666), 2, 1))
        t = np.clip((rx - lo) / (hi - lo), 0.0, 1.0)
        pick = lambda a: np.take_along_axis(a, k[None, :], axis=0)[0]
        d, w1, w2 = pick(self.d), pick(self.c1), pick(self.c2)
        w = w1 / (w1 + w2 * 3.0)
        with np.errstate(all="ignore"):
            tail = t > w
            tt = np.where(tail, np.clip((t - w) / (1.0 - w), 0, 1), np.clip(t / w, 0, 1))
            r = np.where(tail, np.log(1.0 - tt * w2) * (-d * 3.0), np.log(1.0 - tt * w1) * (-d))
        return np.where((self.maxR < EPS) | (d < EPS), 0.0, r)

    def pdf(self, r):
        d = np.maximum(self.d, EPS)
        with np.errstate(all="ignore"):
            s = ((np.exp(-r / d) + np.exp(-r / d / 3.0)) / d / (self.c1 + self.c2 * 3.0)).sum(axis=0)
            p = s / (2.0 * np.pi * r * 3.0)
        return np.where(self.maxR < EPS, 1.0, p)

    def profile(self, r):
        with np.errstate(all="ignore"):
            v = (np.exp(-r / self.d) + np.exp(-r / (3.0 * self.d))) / (8.0 * np.pi * r * self.d)
        v = np.where(self.d < EPS, 1.0, v)
        return np.where(self.maxR < EPS, 0.0, np.where(r < EPS, 1.0, v))


def _lerp(t, a, b):
    return (1.0 - t) * a + t * b


class Disney64:
    """DisneySampler, src/rlDisney.cpp:155-192 (constructor), 199-236 (evalDiffuse), 318-357 (evalSpecular), 359-404
    (samplers), 515-577 (pdfs, D_GTR1, D_GTR2Aniso, smithG_GGX); tangent = mAxisU is an input (AiBuildLocalFramePolar is closed)"""

    def __init__(self, c):
        self.wo, self.N, self.U = (np.asarray(c[k], np.float64) for k in ("wo", "N", "T"))
        n = self.wo.shape[1]
        g = lambda k, d=0.0: np.broadcast_to(np.asarray(c.get(k, d), np.float64), (n,))
        base = np.asarray(c.get("base_color", (1.0, 1.0, 1.0)), np.float64)
        self.base = base if base.ndim == 2 else np.repeat(base[:, None], n, axis=1)
        self.V = np.cross(self.N.T, self.U.T).T
        self.rough, self.subsurface, self.metallic = g("roughness"), g("subsurface"), g("metallic")
        self.specular = g("specular") * float(F(0.08))
        self.clearcoat, self.gloss = g("clearcoat") * 0.25, g("clearcoat_gloss")
        aspect = np.sqrt(1.0 - g("anisotropic") * float(F(0.9)))
        self.ax = np.maximum(float(F(1e-2)), self.rough ** 2 / aspect)
        self.ay = np.maximum(float(F(1e-2)), self.rough ** 2 * aspect)
        self.srough = self.rough ** 2
        lum = self.base[0] * float(F(0.212671)) + self.base[1] * float(F(0.715160)) + self.base[2] * float(F(0.072169))
        tint = np.where(lum > 0, self.base / np.where(lum > 0, lum, 1.0), 1.0)
        metallic_color = self.specular * _lerp(g("specular_tint"), 1.0, tint)
        self.f0 = _lerp(self.metallic, metallic_color, self.base)
        self.sheen_color = _lerp(g("sheen_tint"), 1.0, tint) * g("sheen")

    def _d_gtr2(self, m, mn2):
        hu, hv = (m * self.U).sum(0), (m * self.V).sum(0)
        return (1.0 / np.pi) / (self.ax * self.ay * ((hu / self.ax) ** 2 + (hv / self.ay) ** 2 + mn2) ** 2)

    def _d_gtr1(self, mn2):
        a2 = _lerp(self.gloss, float(F(0.1)), float(F(0.001))) ** 2
        return (a2 - 1.0) / np.pi / (np.log(a2) * (1.0 + (a2 - 1.0) * mn2))

    @staticmethod
    def _smith(nv, a):
        return 1.0 / (nv + np.sqrt(a * a + nv * nv - a * a * nv * nv))

    def eval_diffuse(self, L):
        ln, vn = (L * self.N).sum(0), (self.wo * self.N).sum(0)
        H = _norm(L + self.wo)
        lh, vh = (L * H).sum(0), (self.wo * H).sum(0)                    # the reference names V.H "NdotH" (src/rlDisney.cpp:210)
        black = (ln < EPS) | (vn < EPS) | (vh < EPS) | (lh < EPS)
        fl, fv = np.clip(1.0 - ln, 0, 1) ** 5, np.clip(1.0 - vn, 0, 1) ** 5
        f90 = 0.5 + 2.0 * self.rough * lh * lh
        diffuse = _lerp(fl, 1.0, f90) * _lerp(fv, 1.0, f90)
        fss90 = self.rough * lh * lh
        fss = _lerp(fl, 1.0, fss90) * _lerp(fv, 1.0, fss90)
        with np.errstate(all="ignore"):
            ss = 1.25 * (fss * (1.0 / (ln + vn) - 0.5) + 0.5)
        out = self.base / np.pi * _lerp(self.subsurface, diffuse, ss) * (1.0 - self.metallic)
        return np.where(black, 0.0, out) * ln                           # evalBrdf multiplies by N.L (src/rlDisney.cpp:130-134)

    def eval_specular(self, L):
        ln, vn = (L * self.N).sum(0), (self.wo * self.N).sum(0)
        M = _norm(L + self.wo)
        lm, nm = (L * M).sum(0), (self.N * M).sum(0)
        black = (ln < EPS) | (vn < EPS) | (nm < EPS) | (lm < EPS)
        nm2 = nm * nm
        fh = np.clip(1.0 - lm, 0, 1) ** 5
        with np.errstate(all="ignore"):
            ds, fs = self._d_gtr2(M, nm2), _lerp(fh, self.f0, 1.0)
            gs = self._smith(ln, self.srough) * self._smith(vn, self.srough)
            dr, fr = self._d_gtr1(nm2), _lerp(fh, 0.04, 1.0)
            gr = self._smith(ln, 0.25) * self._smith(vn, 0.25)
            out = ds * fs * gs + self.clearcoat * dr * fr * gr + fh * self.sheen_color * (1.0 - self.metallic)
        return np.where(black, 0.0, out) * ln

    def pdf_diffuse(self, L):
        return np.maximum(EPS, (L * self.N).sum(0) / np.pi)

    def pdf_specular(self, L):
        m = _norm(L + self.wo)
        im, mn = np.abs((L * m).sum(0)), (m * self.N).sum(0)
        cw = self.clearcoat / (self.clearcoat + 1.0)
        vn = np.maximum(1e-4, (self.wo * self.N).sum(0))
        with np.errstate(all="ignore"):
            dw = self._smith(im, self.srough) * self._d_gtr2(m, mn * mn) * 2.0 * im / vn
            d = _lerp(cw, dw, self._d_gtr1(mn * mn) * np.abs(mn) / im)
        return np.where(mn < 0, 0.0, d * 0.25)

    # the explicit sample loop, src/rlDisney.cpp:299-312, for both lobes over the given per-sample directions wi
    # ([3, 2 * spp * n], index lobe * n * spp + s * n + i, lobe 0 = diffuse): a sample counts when its pdf exceeds
    # AI_EPSILON (309) and its direction is not the zero vector; -> sums of evalBrdf / evalPdf and the counts, per lobe
    def integrate(self, spp_n, wi):
        n, spp = self.wo.shape[1], spp_n * spp_n
        out = []
        for lobe, (ev, pd) in enumerate(((self.eval_diffuse, self.pdf_diffuse), (self.eval_specular, self.pdf_specular))):
            total, count = np.zeros((3, n)), np.zeros(n)
            for s in range(spp):
                k = lobe * n * spp + s * n
                w = np.asarray(wi[:, k:k + n], np.float64)
                with np.errstate(all="ignore"):
                    pdf = pd(w)
                    valid = (pdf.astype(F) > F(1e-4)) & ~(w == 0).all(axis=0)
                    total += np.where(valid, ev(w) / pdf, 0.0)
                count += valid
            out += [total, count]
        return tuple(out)


class Sss64:
    """SssSampler<NDProfile>, src/rlSss.h:143-167: the profile and the frame -- U, V from sg->dPdu by Gram-Schmidt (151-154),
    or (has_dPdu false, AiBuildLocalFramePolar being closed) U = the given tangent, V = N x U as Ggx64 builds it.  The scene
    of integrate_scatter is the analytic one rls_sss_scene describes (include/rlshaders_amd.h), given as that struct."""

    def __init__(self, N, T, dist, albedo, has_dPdu=True):
        self.N = np.asarray(N, np.float64)
        self.T = T = np.asarray(T, np.float64)
        n = self.N.shape[1]
        if has_dPdu:
            self.V = _norm(np.cross(self.N.T, _norm(T).T).T)
            self.U = np.cross(self.V.T, self.N.T).T
        else:
            self.U, self.V = T, np.cross(self.N.T, T.T).T
        b3 = lambda v: np.asarray(v, np.float64) if np.ndim(v) == 2 else np.repeat(np.asarray(v, np.float64)[:, None], n, axis=1)
        self.dist32, self.albedo32 = b3(dist).astype(F), b3(albedo).astype(F)
        self.albedo = self.albedo32.astype(np.float64)
        self.nd = NdProfile64(self.dist32)
        self.has_dPdu = has_dPdu

    # the three-axis MIS pdf of a probe hit, src/rlSss.h:252-263 (AiM4Frame + AiM4VectorByMatrixMult as the projection of
    # the displacement onto the frame axes)
    def mis_pdf(self, disp, sampleN):
        o = np.stack([(disp * a).sum(0) for a in (self.U, self.V, self.N)]) ** 2
        rr = np.sqrt(o[1] + o[2]), np.sqrt(o[0] + o[2]), np.sqrt(o[0] + o[1])
        with np.errstate(all="ignore"):
            return sum(self.nd.pdf(r) * np.abs((a * sampleN).sum(0)) * w
                       for r, a, w in zip(rr, (self.U, self.V, self.N), (0.25, 0.25, 0.5)))

    # src/rlSss.h:401-413
    @staticmethod
    def cavity_fade(disp, sampleN, No):
        with np.errstate(all="ignore"):
            d = disp / np.linalg.norm(disp, axis=0)
        c = (sampleN * No).sum(0)
        return np.sqrt((1.0 + np.where((No * d).sum(0) < 0, np.abs(c), np.clip(c, -1.0, 1.0))) * 0.5)

    @staticmethod
    def _trace(sc, O, D, maxdist):
        """the probe ray against the plane or the sphere: a list of (valid, hit point, normal) in ascending distance"""
        v = lambda a: np.asarray(a[:], np.float64)[:, None]
        with np.errstate(all="ignore"):
            if sc.geometry == 0:
                nrm = v(sc.plane_normal)
                t = ((v(sc.plane_point) - O) * nrm).sum(0) / (D * nrm).sum(0)
                ts = [t]
            else:
                oc = O - v(sc.sphere_center)
                b, c = (oc * D).sum(0), (oc * oc).sum(0) - float(sc.sphere_radius) ** 2
                q = np.sqrt(b * b - c)                                      # nan where the ray misses
                ts = [-b - q, -b + q]
            hits = []
            for t in ts:
                P = O + D * t
                N = nrm + 0 * P if sc.geometry == 0 else (P - v(sc.sphere_center)) / float(sc.sphere_radius)
                hits.append(((t > 0) & (t <= maxdist), P, N))
        return hits

    # integrateScatter, src/rlSss.h:227-276, with traceProbe (288-357: hits no farther than AI_EPSILON from the shading point
    # are passed over, 316-317) and shadeProbeSample (379-424: the radius cut-off, the cavity fade, evalLightSample x
    # evalProfile; integrateDiffuse contributes nothing) -> (result [3, n], shaded hits per probe ray [n])
    def integrate_scatter(self, P, scene, spp_n, seed, use_cavity_fade=None, first_index=0, dim_pair=0):
        import oracle_lib as O
        P32 = np.ascontiguousarray(P, F)
        P = P32.astype(np.float64)
        n, spp = P.shape[1], spp_n * spp_n
        fade_on = bool(scene.use_cavity_fade) if use_cavity_fade is None else use_cavity_fade
        v = lambda a: np.asarray(a[:], np.float64)[:, None]
        L, colour = v(scene.light_dir), v(scene.light_color)
        prober = O.Sss(n, self.dist32, self.albedo32, N=self.N.astype(F), T=self.T.astype(F),
                       has_dPdu=self.has_dPdu, nthreads=4)
        acc, depth = np.zeros((3, n)), np.zeros(n)
        for s in range(spp):
            rx, ry = O.batch_sample_02(seed, first_index, n, dim_pair, s)
            pr = prober.probe(rx, ry)                                       # getProbeRay (a33-a34: pinned to the reference)
            org, D = P + pr["origin"].astype(np.float64), pr["dir"].astype(np.float64)
            for ok, hP, hN in self._trace(scene, org, D, pr["maxdist"].astype(np.float64)):
                disp = hP - P
                r = np.linalg.norm(disp, axis=0)
                with np.errstate(all="ignore"):
                    ok = ok & (r.astype(F) > F(1e-4)) & ~(r > self.nd.maxR)
                    fade = self.cavity_fade(disp, hN, self.N) if fade_on else np.ones(n)
                    ok = ok & (fade.astype(F) > F(1e-4))
                    E = colour / np.pi * np.maximum(0.0, (hN * L).sum(0))
                    if scene.has_gate:
                        E = np.where(((hP - v(scene.gate_point)) * v(scene.gate_normal)).sum(0) > 0, E, 0.0)
                    irr = E * self.nd.profile(r) * fade
                    term = irr / self.mis_pdf(disp, hN)
                depth += ok
                acc += np.where(ok & (irr != 0).any(axis=0), term, 0.0)     # AiColorIsZero samples are passed over, 249
        return self.albedo * acc / spp, depth / spp


def _skin_lobe(c, p, name):
    return Ggx64(dict(wo=c["wo"], N=c["N"], T=c["T"], KsColor=p[name + "_color"], roughness=p[name + "_roughness"],
                      ior=p[name + "_ior"], anisotropic=0.0))


def _skin_weights(n, p, sheen_avg, spec_avg):
    """the hand-down of src/rlSkin.cpp:191, 204, 214, 228, 238: thresholds on the fp32 weights"""
    w32 = lambda k: np.broadcast_to(np.asarray(p[k], F), (n,))
    sheen_on, spec_on = w32("sheen_weight") > F(1e-4), w32("specular_weight") > F(1e-4)
    sw, pw, ww = (w32(k).astype(np.float64) for k in ("sheen_weight", "specular_weight", "sss_weight"))
    sheenF = np.where(sheen_on, sheen_avg * sw, 0.0)
    specF = np.where(spec_on, spec_avg * pw, 0.0)
    return sheen_on, spec_on, sw, pw, sheenF, specF, ww * (1.0 - specF * (1.0 - sheenF))


def _skin_dist(n, p):
    d = np.asarray(p["sss_scatter_dist"], F)
    d = d if d.ndim == 2 else np.repeat(d[:, None], n, axis=1)
    return (d * np.broadcast_to(np.asarray(p["sss_dist_multiplier"], F), (n,))).astype(F)     # an fp32 product, src/rlSkin.cpp:236


def skin64(c, p, xi):
    """rlSkin's layer arithmetic with ONE sample per lobe, src/rlSkin.cpp:174-246: per GGX lobe the callback triple and the
    Fresnel term of its one evalSample, the radius sample of the profile, and the three hand-down scalars.  xi: [6, n]"""
    n = np.asarray(c["wo"]).shape[1]
    out = {}
    avg = []
    for name, key, j in (("sheen", "sheen", 0), ("specular", "spec", 2)):
        g = _skin_lobe(c, p, name)
        m = g.microfacet(xi[j], xi[j + 1])
        wi = g.reflect(m)
        out.update({key + "_wi": wi, key + "_f": g.eval(wi), key + "_pdf": g.pdf(wi), key + "_fresnel": g.fresnel(wi, m)})
        avg.append(out[key + "_fresnel"])
    nd = NdProfile64(_skin_dist(n, p))
    # the radius sample as getProbeRay draws it, src/rlSss.h:491-502: rx stretched over its axis interval first (exact in fp32)
    rx = np.asarray(xi[4], F)
    rx = np.where(rx < F(0.5), rx / F(0.5), np.where(rx < F(0.75), (rx - F(0.5)) / F(0.25), (rx - F(0.75)) / F(0.25))).astype(F)
    out["r"] = nd.radius(rx)
    out["r_pdf"], out["profile"] = nd.pdf(out["r"]), nd.profile(out["r"])
    on = dict(zip(("sheen", "spec"), _skin_weights(n, p, avg[0], avg[1])[:2]))
    out["sheenFresnel"], out["specularFresnel"], out["sssWeight"] = _skin_weights(n, p, avg[0], avg[1])[4:]
    for key, mask in on.items():                                            # a lobe at or below the weight threshold is never built
        for k in ("_wi", "_f", "_pdf", "_fresnel"):
            out[key + k] = np.where(mask, out[key + k], 0.0)
    for k in ("r", "r_pdf", "profile"):                                     # nor is a radius drawn below the switch of 244
        out[k] = np.where(out["sssWeight"].astype(F) < F(1e-4), 0.0, out[k])
    return out


def skin_integrate64(c, p, P, scene, spp_n, seed, env=(1.0, 1.0, 1.0), first_index=0):
    """shader_evaluate of rlSkin without lights over spp_n^2 samples per layer, src/rlSkin.cpp:174-254: integrateGlossy per
    lobe (the closed AiBRDFIntegrate as the mean of evalBrdf / evalPdf x a uniform environment), getAvgReflectWeight handed
    down 204 -> 231 -> 238, the small-weight switch 244, scatter x weight, the sum 254.  Sample streams 0, 1, 2."""
    n = np.asarray(c["wo"]).shape[1]
    spp = spp_n * spp_n
    env = np.asarray(env, np.float64)[:, None]
    ssum, savg = _skin_lobe(c, p, "sheen").integrate(spp_n, seed, first_index, dim_pair=0)
    psum, pavg = _skin_lobe(c, p, "specular").integrate(spp_n, seed, first_index, dim_pair=1)
    sheen_on, spec_on, sw, pw, sheenF, specF, sssW = _skin_weights(n, p, savg, pavg)
    sheen = np.where(sheen_on, env * ssum / spp, 0.0) * sw
    specular = np.where(spec_on, env * psum / spp, 0.0) * (pw * (1.0 - sheenF))
    col = np.asarray(p["sss_color"], np.float64)
    scatter, _ = Sss64(c["N"], c["T"], _skin_dist(n, p), col).integrate_scatter(P, scene, spp_n, seed, None, first_index, 2)
    sss = np.where(sssW.astype(F) < F(1e-4), 0.0, scatter * sssW)
    return dict(sheen=sheen, specular=specular, sss=sss, out=sheen + specular + sss, sheenFresnel=sheenF,
                specularFresnel=specF, sssWeight=sssW)
