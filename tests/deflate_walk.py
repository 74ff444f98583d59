"""A block and token walker for raw DEFLATE streams, on top of tests/inflate_ref.py (its tables, its canonical codes, its verdict on a code
set): what an ENCODER's output is held against.  walk(src) returns (blocks, used): per block its type, whether it is final, and its tokens
-- ("lit", byte) / ("match", length, distance, length symbol) -- or, for a stored block, its LEN; `used` is the number of bytes up to the
end of the final block.  Anything the reference decoder would refuse raises ValueError.  Fields are cut out of an 8-byte window, so a walk
costs a few operations per token, not per bit."""
import inflate_ref as R

STORED, FIXED, DYNAMIC = 0, 1, 2


class _Reader:
    def __init__(self, src):
        self.src, self.pos, self.nbits = src + bytes(8), 0, 8 * len(src)

    def _window(self):
        """the next 57 bits at least (zeros behind the end)"""
        at = self.pos >> 3
        return int.from_bytes(self.src[at:at + 8], "little") >> (self.pos & 7)

    def get(self, n):
        if self.pos + n > self.nbits:
            raise ValueError("the stream ends inside a field")
        v = self._window() & ((1 << n) - 1)
        self.pos += n
        return v

    def peek15(self):
        return self._window() & 0x7FFF


class _Code:
    def __init__(self, lens, codes_kind=False):
        try:
            R._check_set(lens, codes_kind)
        except R._Bad:
            raise ValueError("a code set the decoder refuses: %r" % (lens,))
        self.by = {(l, c): s for s, (c, l) in R.canonical(lens).items()}
        self.maxl = max([l for l in lens if l], default=0)

    def read(self, rd):
        v, c = rd.peek15(), 0
        for l in range(1, self.maxl + 1):
            c = (c << 1) | ((v >> (l - 1)) & 1)
            s = self.by.get((l, c))
            if s is not None:
                rd.get(l)
                return s
        raise ValueError("a code the set does not have")


_FIXED = None


def walk(src):
    global _FIXED
    if _FIXED is None:
        _FIXED = (_Code(R.FIXED_LIT), _Code(R.FIXED_DIST))
    rd, blocks, produced = _Reader(bytes(src)), [], 0
    while True:
        final, btype = rd.get(1), rd.get(2)
        if btype == 3:
            raise ValueError("block type 3")
        blk = dict(type=btype, final=final, tokens=[], stored=None, start=produced)
        blocks.append(blk)
        if btype == STORED:
            rd.pos = (rd.pos + 7) & ~7
            n, nn = rd.get(16), rd.get(16)
            if n ^ 0xFFFF != nn:
                raise ValueError("NLEN")
            if rd.pos + 8 * n > rd.nbits:
                raise ValueError("a stored block runs past the end")
            rd.pos += 8 * n
            blk["stored"] = n
            produced += n
        else:
            if btype == FIXED:
                lit, dist = _FIXED
            else:
                nlen, ndist, ncl = rd.get(5) + 257, rd.get(5) + 1, rd.get(4) + 4
                if nlen > 286 or ndist > 30:
                    raise ValueError("HLIT / HDIST")
                cl_lens = [0] * 19
                for i in range(ncl):
                    cl_lens[R.CL_ORDER[i]] = rd.get(3)
                cl, lens = _Code(cl_lens, True), []
                while len(lens) < nlen + ndist:
                    s = cl.read(rd)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16 and not lens:
                        raise ValueError("repeat with nothing in front of it")
                    rep = (3, 3, 11)[s - 16] + rd.get((2, 3, 7)[s - 16])
                    if len(lens) + rep > nlen + ndist:
                        raise ValueError("a repeat runs past the lengths")
                    lens += [lens[-1] if s == 16 else 0] * rep
                if lens[256] == 0:
                    raise ValueError("no end-of-block code")
                lit, dist = _Code(lens[:nlen]), _Code(lens[nlen:])
            while True:
                s = lit.read(rd)
                if s < 256:
                    blk["tokens"].append(("lit", s))
                    produced += 1
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol %d" % s)
                    length = R.LEN_BASE[s - 257] + rd.get(R.LEN_EXTRA[s - 257])
                    d = dist.read(rd)
                    if d > 29:
                        raise ValueError("distance symbol %d" % d)
                    distance = R.DIST_BASE[d] + rd.get(R.DIST_EXTRA[d])
                    if distance > produced:
                        raise ValueError("distance %d at position %d" % (distance, produced))
                    blk["tokens"].append(("match", length, distance, s))
                    produced += length
        if final:
            return blocks, (rd.pos + 7) >> 3
