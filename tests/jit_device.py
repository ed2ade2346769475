"""One case of tests/jit_cases.py on the device, through the C ABI (``pdehip_jit_apply`` / ``pdehip_jit_apply_stage``): every array of the call is
uploaded as a whole allocation (a pattern of distinct values with the case's cells in their places), read back whole and compared element by
element - written cells against the reference, everything else against the upload.  Used by tests/test_hip_jit_instances.py and, in a process of
its own with the tuning knobs set, by tests/jit_knob_worker.py."""

from __future__ import annotations

import ctypes as C

import jit_cases as J
import numpy as np
import small_kernel_cases as S

from pde_hip import _abi
from pde_hip.device import DeviceBuffer, GridInfo
from pde_hip.faces import _upload_f64

BASES = {"in": 1024, "e0": 3000, "e1": 5000, "e2": 7000, "y": 9000, "k0": 11000, "k1": 13000, "k2": 15000, "k3": 17000, "k4": 19000, "out": 21000, "out2": 23000}
MARK_SHAPE = (4, 8)


def differences(got, ref, what):
    """"" when two flat images agree: NaNs by position (payloads are not compared), every other element by its bits."""
    got, ref = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(ref).ravel()
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    bad = np.flatnonzero((nan_g != nan_r) | ((S.bits(got) != S.bits(ref)) & ~nan_r))
    if not bad.size:
        return ""
    at = int(bad[0])
    return f"{what}: {bad.size} of {got.size} elements differ, first at element {at}: {got[at]!r} != {ref[at]!r}"


class Runner:
    def __init__(self, lib, knobs=None):
        self.lib, self.knobs = lib, knobs
        self.handles, self.infos = {}, {}
        self.calls = 0

    def handle(self, body):
        if body not in self.handles:
            h = C.c_void_p()
            if isinstance(body, tuple):     # (level 1, level 2) of a fused two-pass expression
                self.lib.jit_create2(J.ALL_BODIES[body[0]][0].encode(), J.ALL_BODIES[body[1]][0].encode(), C.byref(h))
            else:
                self.lib.jit_create(J.ALL_BODIES[body][0].encode(), C.byref(h))
            self.handles[body] = h
        return self.handles[body]

    def info(self, shape, dtype):
        key = (tuple(shape), np.dtype(dtype).str)
        if key not in self.infos:
            info = GridInfo(shape, J.DX[3 - len(shape):], dtype)
            lay = S.Layout(shape, dtype)
            eight = (C.c_int64 * 8)()
            self.lib.layout(info.ref, eight)
            assert list(eight) == lay.eight(), f"pdehip_layout {list(eight)} != the documented rule {lay.eight()}"
            self.infos[key] = (info, lay)
        return self.infos[key]

    # ---- the mark: a launch no case uses (2-D, ghost cells preset, fp64, one tile), so that a call that records nothing shows
    def mark(self):
        info, lay = self.info(MARK_SHAPE, np.float64)
        if not hasattr(self, "_mark"):
            img = S.image(lay, 1)
            self._mark = (self.upload(img), self.upload(img))
        self.lib.jit_apply(self.handle("kpz"), info.ref, self._mark[0].ptr, None, self._mark[1].ptr, J._pd(J.PARAMS), 3, None, None)
        name = J.kernel_name(J.plan(MARK_SHAPE, np.float64, knobs=self.knobs))
        got = self.lib.last_kernel_name().decode()
        assert got == name, f"the mark: {got!r} != {name!r}"
        return name

    def upload(self, img, shift=0):
        buf = DeviceBuffer(img.nbytes + 2 * shift)
        buf.at = buf.ptr + shift
        assert buf.ptr % 16 == 0 and buf.at % 16 == shift
        self.lib.memcpy_h2d(buf.at, img.ctypes.data, img.nbytes, None)
        return buf

    def read(self, buf, like):
        out = np.empty_like(like)
        self.lib.memcpy_d2h(out.ctypes.data, buf.at if hasattr(buf, "at") else buf.ptr, out.nbytes, None)
        return out

    def run(self, c, stage_on_generic=False):
        """-> (name recorded, list of differences); ``stage_on_generic``: the stage entry point on a misaligned case (must launch nothing)."""
        lib = self.lib
        p = J.case_plan(c, self.knobs)
        a = J.arrays(c, p)
        st = c.stage if not c.shift else ({"kind": 0, "nk": 1} if stage_on_generic else None)
        if c.shift and stage_on_generic:
            a["y"], a["k0"] = a["e0"], a["e1"]
        info, lay = self.info(c.shape, c.dtype)
        nd = len(c.shape)
        inner = S.interior(nd)
        ref = {"k": None, "out2": None, "err": None} if (c.shift and stage_on_generic) else J.reference(c, a)
        # ---- images before the call
        img = {}
        for role, arr in a.items():
            whole = role != "in" or c.faces == "preset"
            src = J.with_ghosts(c, a) if (role == "in" and c.faces == "preset") else arr
            img[role] = S.place(S.pattern(lay.nelem(1), lay.dtype, base=BASES[role]), lay, 1, src.reshape(1, *src.shape), None if whole else inner)
        img["out"] = S.pattern(lay.nelem(1), lay.dtype, sign=1.0, base=BASES["out"])
        if st is not None and st.get("alias") != "out2=y":
            img["out2"] = S.pattern(lay.nelem(1), lay.dtype, sign=1.0, base=BASES["out2"])
        shifted = {"in": "in", "out": "out", "extra": "e1"}.get(c.shift)
        dev = {role: self.upload(im, 8 if role == shifted else 0) for role, im in img.items()}
        errbuf = self.upload(S.pattern(8, np.float64, base=500))
        # ---- the call
        table = None if c.faces == "preset" else S.face_table(J.face_list(c.shape, c.faces), upload=_upload_f64)
        ex = (C.c_void_p * 3)(*[dev[f"e{m}"].at if f"e{m}" in dev else None for m in range(3)])
        nparams = J.BODIES[c.body][1]
        mark = self.mark()
        done = C.c_int(-1)
        if st is None:
            lib.jit_apply(self.handle(c.body), info.ref, dev["in"].at, ex, dev["out"].at, J._pd(J.PARAMS), nparams, table, None)
        else:
            ks = [dev["in"].at if (st.get("alias") == "k1=in" and m == 1) else dev[f"k{m}"].at for m in range(st["nk"])]
            kp = (C.c_void_p * 5)(*ks)
            cf = J._pd([J.DT4, 0.0] if st["kind"] == 4 else [*J.COEF[: st["nk"]], 0.0])
            out2 = dev["y"].at if st.get("alias") == "out2=y" else dev["out2"].at
            lib.jit_apply_stage(self.handle(c.body), info.ref, dev["in"].at, ex, dev["out"].at, J._pd(J.PARAMS), nparams, table, st["kind"], dev["y"].at,
                                st["nk"], kp, cf, J.C_NEW, out2, errbuf.at if st["kind"] in (2, 4) else None, C.byref(done), None)
        name = lib.last_kernel_name().decode()
        self.calls += 1
        # ---- what the allocations must hold now
        want = {role: im.copy() for role, im in img.items()}
        launched = not (c.shift and stage_on_generic)
        bad = []
        if st is not None and done.value != (1 if launched else 0):
            bad.append(f"*done = {done.value}")
        if launched:
            if name != J.kernel_name(p):
                bad.append(f"name {name!r}, expected {J.kernel_name(p)!r}")
            after = J.input_after_call(c, a, p.generic)
            changed = S.bits(after) != S.bits(a["in"])
            if changed.any():
                want["in"][lay.index_full()[changed]] = after[changed]
            if ref["k"] is not None:
                S.place(want["out"], lay, 1, ref["k"].reshape(1, *ref["k"].shape), inner)
            if ref["out2"] is not None:
                S.place(want["y" if st.get("alias") == "out2=y" else "out2"], lay, 1, ref["out2"].reshape(1, *ref["out2"].shape), inner)
        elif name != mark:
            bad.append(f"a call that launches nothing recorded {name!r}")
        for role in img:
            d = differences(self.read(dev[role], img[role]), want[role], f"array {role} (whole allocation)")
            if d:
                bad.append(d)
        err = self.read(errbuf, np.empty(8, np.float64))
        want_err = S.pattern(8, np.float64, base=500)
        if launched and st is not None and st["kind"] in (2, 4):
            want_err[0] = ref["err"]
        d = differences(err, want_err, "the error cell and the seven doubles behind it")
        if d:
            bad.append(d)
        return name, bad

    def run_two_level(self, mode, dtype, shape, ry):
        """pdehip_jit_euler2 ("two") / pdehip_jit_fused2 ("fused2") on one grid with walls on every face -> (name, differences)"""
        lib = self.lib
        info, lay = self.info(shape, dtype)
        inner = S.interior(len(shape))
        src, ref = J.two_level_reference(mode, dtype, shape)
        img_in = S.place(S.pattern(lay.nelem(1), lay.dtype, base=BASES["in"]), lay, 1, src.reshape(1, *src.shape), inner)
        img_out = S.pattern(lay.nelem(1), lay.dtype, sign=1.0, base=BASES["out"])
        d_in, d_out = self.upload(img_in), self.upload(img_out)
        table = S.face_table(J.face_list(shape, "walls"), upload=_upload_f64)
        mark = self.mark()
        done = C.c_int(-1)
        if mode == "two":
            lib.jit_euler2(self.handle("euler_update"), info.ref, d_in.at, d_out.at, J._pd(J.PARAMS), 3, table, C.byref(done), None)
        else:
            lib.jit_fused2(self.handle(("chain_first", "chain_second")), info.ref, d_in.at, d_out.at, J._pd(J.PARAMS), 3, table, table, C.byref(done), None)
        name = lib.last_kernel_name().decode()
        bad = []
        if done.value != 1:
            bad.append(f"*done = {done.value} (name {name!r}, mark {mark!r})")
            return name, bad
        if name != J.two_level_name(mode, dtype, shape, ry):
            bad.append(f"name {name!r}, expected {J.two_level_name(mode, dtype, shape, ry)!r}")
        want = S.place(img_out.copy(), lay, 1, ref.reshape(1, *ref.shape), inner)
        for what, dev, image in (("input", d_in, img_in), ("output", d_out, want)):
            d = differences(self.read(dev, image), image, f"{what} (whole allocation)")
            if d:
                bad.append(d)
        return name, bad
