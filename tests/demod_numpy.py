"""The demod.java chain (demod.java:341-483) restated in numpy float32, one operation at a time: what tests/test_demod.py holds
the oracle to and tests/test_demod_host.py the library's host unit (weights, the carrier phase)."""
import numpy as np

f32 = np.float32


def java_short_of_float(v):
    v = f32(v)
    if np.isnan(v):
        i = 0
    elif v >= f32(2147483648.0):
        i = 2147483647
    elif v <= f32(-2147483648.0):
        i = -2147483648
    else:
        i = int(np.trunc(v))
    return ((i + 32768) & 0xFFFF) - 32768


class NumpyDemod:
    """written from the Java text, one float32 operation at a time"""

    def __init__(self, rate):
        self.rate = rate
        self.mode = self.dofir = self.dodwn = self.doagc = 0
        self.fir = np.zeros(42, f32)
        self.wfir = np.zeros(21, f32)
        self.fof = 0
        self.car = f32(0)
        self.phi = f32(0)
        self.li = f32(0)
        self.lq = f32(0)

    def weights(self, flo, fhi):
        rate = f32(self.rate)
        nlo = f32(flo) / rate
        nhi = f32(fhi) / rate
        for n in range(21):
            if n == 10:
                self.wfir[n] = f32(2) * (nhi - nlo)
            else:
                k = float(n - 10)
                self.wfir[n] = f32(np.sin(2 * np.pi * float(nhi) * k) / (np.pi * k) - np.sin(2 * np.pi * float(nlo) * k) / (np.pi * k))
            self.wfir[n] = self.wfir[n] * f32(0.54 - 0.46 * np.cos(2 * np.pi * n / 20.0))
        self.phi = f32(2 * np.pi * float(nlo))
        self.car = f32(0)
        self.fir[:] = 0
        self.fof = 40

    def step_car(self):
        """:427-429"""
        self.car = self.car - self.phi
        if self.car < 0:
            self.car = self.car + f32(2 * np.pi)

    def receive(self, buf):
        n2 = buf.size
        sam = np.zeros(n2, f32)
        mx = f32(0)
        avg = f32(0)
        fmgain = f32(self.rate) / (f32(5000) if self.mode == 3 else f32(75000))
        for s in range(0, n2, 2):
            i, q = f32(buf[s]), f32(buf[s + 1])
            if self.dofir:
                self.fir[self.fof] = i
                self.fir[self.fof + 1] = q
                oi = f32(0)
                oq = f32(0)
                for t in range(0, 42, 2):
                    ti = (self.fof + t) % 42
                    oi = oi + self.fir[ti] * self.wfir[t // 2]
                    oq = oq + self.fir[ti + 1] * self.wfir[t // 2]
                i, q = oi, oq
                self.fof -= 2
                if self.fof < 0:
                    self.fof = 40
            if self.dodwn:
                ci = f32(np.cos(float(self.car)))
                cq = f32(np.sin(float(self.car)))
                self.step_car()
                i, q = i * ci - q * cq, i * cq + q * ci
            if self.mode == 0:
                i = f32(0)
            elif self.mode == 2:
                i = f32(np.sqrt(float(i * i + q * q)))
                avg = (f32(s // 2) * avg + i) / f32(s // 2 + 1)
            elif self.mode in (3, 4):
                v = ((self.li * q) - (self.lq * i)) * fmgain
                self.li, self.lq = i, q
                i = v
            sam[s] = i
            a = np.abs(i)
            mx = f32(np.nan) if (np.isnan(mx) or np.isnan(a)) else max(mx, a)
        if self.mode == 2:
            mx = mx - avg
        out = np.zeros(n2, np.int16)
        with np.errstate(all="ignore"):
            for s in range(0, n2, 2):
                v = (sam[s] - avg if self.mode == 2 else sam[s]) * (f32(1) / mx if self.doagc else f32(1))
                out[s] = out[s + 1] = java_short_of_float(v * f32(32767))
        return out, mx, avg
