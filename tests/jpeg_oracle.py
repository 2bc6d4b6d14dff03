"""numpy restatement of the JPEG decoder of include/ssd_hip.h: marker parsing, Huffman decoding, the refusals, and the
reconstruction arithmetic (int64 throughout).  Written for clarity, not speed: bit by bit, block by block.

    header(data)          -> dict(width, height, ncomp, kind, blocks_w, blocks_h, ncoef, restart, coef_off, qt [ncomp,64])
    entropy_decode(data)  -> (coef int16 [ncoef], header)
    reconstruct(coef, h)  -> uint8 [H, W, 3]
    decode(data)          -> uint8 [H, W, 3]
Unsupported / Corrupt are raised where the library returns SSD_ERR_UNSUPPORTED / SSD_ERR_VALUE."""
import numpy as np

GREY, K444, K422, K420 = 0, 1, 2, 3


class Unsupported(Exception):
    status = -5


class Corrupt(Exception):
    status = -2


def _zigzag():
    order, x, y, up = [], 0, 0, True
    for _ in range(64):
        order.append(8 * y + x)
        if up:
            if x == 7:
                y, up = y + 1, False
            elif y == 0:
                x, up = x + 1, False
            else:
                x, y = x + 1, y - 1
        else:
            if y == 7:
                x, up = x + 1, True
            elif x == 0:
                y, up = y + 1, True
            else:
                x, y = x - 1, y + 1
    return order


ZIGZAG = _zigzag()


def _huff_table(counts, symbols):
    """{(length, code): symbol}; Corrupt for an over-subscribed table"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= 1 << length:
                raise Corrupt("over-subscribed Huffman table")
            table[(length, code)] = symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def _parse(d):
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Corrupt("no SOI")
    p = 2
    f = dict(restart=0)
    qt, dc, ac = {}, {}, {}
    jfif = adobe = False
    transform = 0
    while True:
        if p + 2 > n or d[p] != 0xFF:
            raise Corrupt("no marker where one must stand")
        while p + 1 < n and d[p + 1] == 0xFF:
            p += 1
        if p + 2 > n:
            raise Corrupt("ran out of data")
        m = d[p + 1]
        p += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Corrupt("EOI before a scan")
        if p + 2 > n:
            raise Corrupt("ran out of data")
        length = (d[p] << 8) | d[p + 1]
        if length < 2 or p + length > n:
            raise Corrupt("segment length past the end")
        s = d[p + 2:p + length]
        if m == 0xC0:
            if "width" in f or len(s) < 6:
                raise Corrupt("bad SOF")
            if s[0] != 8:
                raise Unsupported("precision %d" % s[0])
            f["height"], f["width"], f["ncomp"] = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if f["ncomp"] == 0:
                raise Corrupt("no components")
            if f["ncomp"] not in (1, 3):
                raise Unsupported("%d components" % f["ncomp"])
            if len(s) < 6 + 3 * f["ncomp"]:
                raise Corrupt("short SOF")
            if f["width"] == 0 or f["height"] == 0:
                raise Corrupt("zero dimension")
            f["ids"] = [s[6 + 3 * c] for c in range(f["ncomp"])]
            f["hs"] = [s[7 + 3 * c] >> 4 for c in range(f["ncomp"])]
            f["vs"] = [s[7 + 3 * c] & 15 for c in range(f["ncomp"])]
            f["tq"] = [s[8 + 3 * c] for c in range(f["ncomp"])]
            if any(not 1 <= v <= 4 for v in f["hs"] + f["vs"]) or any(t > 3 for t in f["tq"]):
                raise Corrupt("bad sampling factor or table id")
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported("frame type %#x" % m)
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if q + 17 > len(s):
                    raise Corrupt("short DHT")
                tc, th = s[q] >> 4, s[q] & 15
                counts = list(s[q + 1:q + 17])
                if tc > 1 or th > 3 or sum(counts) > 256 or q + 17 + sum(counts) > len(s):
                    raise Corrupt("bad DHT")
                (ac if tc else dc)[th] = _huff_table(counts, list(s[q + 17:q + 17 + sum(counts)]))
                q += 17 + sum(counts)
        elif m == 0xDB:
            q = 0
            while q < len(s):
                pq, tq = s[q] >> 4, s[q] & 15
                if tq > 3 or pq > 1:
                    raise Corrupt("bad DQT")
                if pq == 1:
                    raise Unsupported("16-bit quantisation table")
                if q + 65 > len(s):
                    raise Corrupt("short DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(s[q + 1:q + 65])
                qt[tq] = t
                q += 65
        elif m == 0xDD:
            if len(s) < 2:
                raise Corrupt("short DRI")
            f["restart"] = (s[0] << 8) | s[1]
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe, transform = True, s[11]
        elif m == 0xDC:
            raise Unsupported("DNL")
        elif m == 0xDA:
            if "width" not in f or len(s) < 1:
                raise Corrupt("scan before frame")
            ns = s[0]
            if not 1 <= ns <= 4 or len(s) < 4 + 2 * ns:
                raise Corrupt("bad SOS")
            if ns != f["ncomp"]:
                raise Unsupported("multi-scan")
            f["td"], f["ta"] = [], []
            for c in range(ns):
                if s[1 + 2 * c] != f["ids"][c]:
                    raise Unsupported("scan order")
                f["td"].append(s[2 + 2 * c] >> 4)
                f["ta"].append(s[2 + 2 * c] & 15)
            if max(f["td"] + f["ta"]) > 3:
                raise Corrupt("bad table id")
            if (s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]) != (0, 63, 0):
                raise Corrupt("not a baseline scan")
            p += length
            break
        p += length
    f["scan"] = p
    if f["ncomp"] == 1:
        f["kind"], f["hs"], f["vs"] = GREY, [1], [1]
    else:
        if (f["hs"][1], f["vs"][1], f["hs"][2], f["vs"][2]) != (1, 1, 1, 1):
            raise Unsupported("chroma sampling")
        kinds = {(1, 1): K444, (2, 1): K422, (2, 2): K420}
        if (f["hs"][0], f["vs"][0]) not in kinds:
            raise Unsupported("luma sampling")
        f["kind"] = kinds[(f["hs"][0], f["vs"][0])]
        rgb = False if jfif else (transform == 0 if adobe else f["ids"] == [82, 71, 66])
        if rgb:
            raise Unsupported("RGB-marked stream")
    f["mcus_x"] = -(-f["width"] // (8 * f["hs"][0]))
    f["mcus_y"] = -(-f["height"] // (8 * f["vs"][0]))
    f["blocks_w"], f["blocks_h"], f["coef_off"], total = [], [], [], 0
    for c in range(f["ncomp"]):
        if f["tq"][c] not in qt or f["td"][c] not in dc or f["ta"][c] not in ac:
            raise Corrupt("missing table")
        f["blocks_w"].append(f["mcus_x"] * f["hs"][c])
        f["blocks_h"].append(f["mcus_y"] * f["vs"][c])
        f["coef_off"].append(total)
        total += 64 * f["blocks_w"][c] * f["blocks_h"][c]
    f["ncoef"] = total
    f["qt"] = np.stack([qt[f["tq"][c]] for c in range(f["ncomp"])])
    f["dc"], f["ac"] = [dc[t] for t in f["td"]], [ac[t] for t in f["ta"]]
    return f


_PUBLIC = ("width", "height", "ncomp", "kind", "blocks_w", "blocks_h", "ncoef", "restart", "coef_off", "qt")


def header(data):
    f = _parse(bytes(data))
    return {k: f[k] for k in _PUBLIC}


class _Bits:
    """bit by bit: position p, bit index in the current byte; past a marker or the end of the data there is nothing to read"""

    def __init__(self, d, p):
        self.d, self.p, self.bit = d, p, 0

    def _byte(self):
        d, p = self.d, self.p
        while True:
            if p >= len(d):
                raise Corrupt("entropy data ends early")
            if d[p] != 0xFF:
                return d[p]
            if p + 1 >= len(d):
                raise Corrupt("entropy data ends early")
            if d[p + 1] == 0x00:
                return 0xFF
            if d[p + 1] == 0xFF:
                p += 1
                self.p = p
                continue
            raise Corrupt("marker %#x inside entropy data" % d[p + 1])

    def get(self):
        b = self._byte()
        v = (b >> (7 - self.bit)) & 1
        self.bit += 1
        if self.bit == 8:
            self.bit = 0
            self.p += 2 if self.d[self.p] == 0xFF else 1
        return v

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.get()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get()
            if (length, code) in table:
                return table[(length, code)]
        raise Corrupt("Huffman code not in the table")

    def align(self):
        """drop the padding bits; returns the offset of the byte that follows (fill bytes skipped)"""
        if self.bit:
            self.bit = 0
            self.p += 2 if self.d[self.p] == 0xFF else 1
        return self.p


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy_decode(data):
    d = bytes(data)
    f = _parse(d)
    coef = np.zeros(f["ncoef"], np.int64)
    b = _Bits(d, f["scan"])
    pred = [0] * f["ncomp"]
    mcus, done, rst = f["mcus_x"] * f["mcus_y"], 0, 0
    for my in range(f["mcus_y"]):
        for mx in range(f["mcus_x"]):
            for c in range(f["ncomp"]):
                for v in range(f["vs"][c]):
                    for h in range(f["hs"][c]):
                        blk = (my * f["vs"][c] + v) * f["blocks_w"][c] + mx * f["hs"][c] + h
                        out = coef[f["coef_off"][c] + 64 * blk:][:64]
                        s = b.symbol(f["dc"][c])
                        if s > 15:
                            raise Corrupt("DC category")
                        if s:
                            pred[c] += _extend(b.bits(s), s)
                        out[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = b.symbol(f["ac"][c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                if k > 64:
                                    raise Corrupt("coefficient index past 63")
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt("coefficient index past 63")
                            out[ZIGZAG[k]] = _extend(b.bits(s), s)
                            k += 1
            done += 1
            if f["restart"] and done % f["restart"] == 0 and done < mcus:
                p = b.align()
                while p + 1 < len(d) and d[p] == 0xFF and d[p + 1] == 0xFF:
                    p += 1
                if p + 1 >= len(d) or d[p] != 0xFF or d[p + 1] != 0xD0 + rst:
                    raise Corrupt("missing or wrong restart marker")
                rst = (rst + 1) & 7
                b = _Bits(d, p + 2)
                pred = [0] * f["ncomp"]
    p = b.align()
    while True:                                    # the first marker behind the last MCU must be EOI
        if p + 1 >= len(d):
            raise Corrupt("no EOI behind the scan")
        if d[p] == 0xFF and d[p + 1] not in (0x00, 0xFF):
            if d[p + 1] != 0xD9:
                raise Corrupt("another marker where EOI must stand")
            break
        p += 2 if d[p] == 0xFF and d[p + 1] == 0x00 else 1
    return ((coef + 32768) % 65536 - 32768).astype(np.int16), {k: f[k] for k in _PUBLIC}


def _ds(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, shift):
    """d: int64 [..., 8] along the last axis"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    z1 = (d2 + d6) * 4433
    t2, t3 = z1 - d6 * 15137, z1 + d2 * 6270
    t0, t1 = (d0 + d4) << 13, (d0 - d4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = d7, d5, d3, d1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return np.stack([_ds(v, shift) for v in (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)], -1)


def planes(coef, h):
    """the padded uint8 sample plane of every component (as int64 arrays)"""
    out = []
    for c in range(h["ncomp"]):
        bw, bh = h["blocks_w"][c], h["blocks_h"][c]
        blk = np.asarray(coef[h["coef_off"][c]:][:64 * bw * bh], np.int64).reshape(bh, bw, 8, 8) * h["qt"][c].reshape(8, 8)
        cols = _idct_pass(blk.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # along each column
        rows = _idct_pass(cols, 18)                                           # along each row
        out.append(np.clip(rows + 128, 0, 255).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _up_h(p):
    """triangle filter along the last axis, 2x (libjpeg h2v1 fancy); p int64 [rows, cw], cw > 2"""
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], -1).reshape(p.shape[0], -1)


def _up_hv(p):
    """2x2 (libjpeg h2v2 fancy); p int64 [ch, cw], cw > 2"""
    above, below = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    r = np.stack([3 * p + above, 3 * p + below], 1).reshape(-1, p.shape[1])    # rows 2j, 2j+1
    left, right = np.concatenate([r[:, :1], r[:, :-1]], 1), np.concatenate([r[:, 1:], r[:, -1:]], 1)
    even, odd = (3 * r + left + 8) >> 4, (3 * r + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * r[:, 0] + 8) >> 4, (4 * r[:, -1] + 7) >> 4
    return np.stack([even, odd], -1).reshape(r.shape[0], -1)


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct(coef, h):
    W, H, kind = h["width"], h["height"], h["kind"]
    pl = planes(coef, h)
    Y = pl[0][:H, :W]
    if kind == GREY:
        return np.stack([Y, Y, Y], -1).astype(np.uint8)
    chroma = []
    for p in pl[1:]:
        if kind == K444:
            c = p[:H, :W]
        else:
            cw, ch = (W + 1) // 2, (H + 1) // 2 if kind == K420 else H
            p = p[:ch, :cw]
            if cw <= 2:                                           # libjpeg: replication for planes of one or two columns
                c = np.repeat(np.repeat(p, 2, 1), 2 if kind == K420 else 1, 0)
            else:
                c = _up_h(p) if kind == K422 else _up_hv(p)
            c = c[:H, :W]
        chroma.append(c - 128)
    cb, cr = chroma
    R = Y + ((_fix(1.402) * cr + 32768) >> 16)
    G = Y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    B = Y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


def decode(data):
    coef, h = entropy_decode(data)
    return reconstruct(coef, h)
