"""Pure-Python restatement of the reference's match finder (src/AuroraLib.Compression/MatchFinder/LzChainMatchFinder.cs:13-372) and of
FlagWriter (IO/FlagWriter.cs:13-147).  TEST-ONLY.  The CPU oracle has no CRILAYLA and no ALLZ body, so the yardstick of the alz_bitenc_* tests is
this finder under the two CompressHeaderless bodies of tests/bitenc_ref.py; the finder itself is pinned to the oracle through formats the oracle
does have (tests/test_bitenc_cpu.py: LZ10, Yaz0 and, for the LzProperties[] form, RefPack).  It follows the C# method by method -- the real head,
chain and min-length tables with their masks, not the prev() identity the kernels use -- and is not fast; the hashes of all positions are
computed at once with numpy, everything else is the managed loop.

ChainFinder(props, quality, max_window_bits=0, strategy=0).find_next_best_match(data) -> (offset, distance, length), (len(data), 0, 0) at the end.
matches(props, data, quality, ...) -> the whole list, the end entry included."""
import math

import numpy as np

M32 = 0xFFFFFFFF
PRIME = 2654435761


class LzProperties:
    """LzProperties(windowsSize, maxLength, minLength = 3, windowsStart = 0, minDistance = 1)  LzProperties.cs:46-55"""

    def __init__(self, window_size, max_length, min_length=3, windows_start=0, min_distance=1):
        self.WindowsBits = math.ceil(math.log2(window_size))
        self.MinLength, self.MaxLength = min_length, max_length
        self.MaxDistance, self.MinDistance = window_size, min_distance


def get_max_chain(quality):              # :111-119
    if quality < 6:
        return quality + 1
    if quality >= 11:
        return 1 << (quality - 5)
    base = 1 << (quality >> 1)
    return base | (base >> (quality & 1))


def match_length(data, a, b, mx):
    """GetMatchLength(dataA = data + a, dataB = data + b, max)  :338-357 (in slices of 64 bytes instead of 8: the same count)"""
    n = 0
    while n < mx:
        k = min(64, mx - n)
        if data[a + n:a + n + k] == data[b + n:b + n + k]:
            n += k
            continue
        while data[a + n] == data[b + n]:
            n += 1
        return n
    return n


class ChainFinder:
    def __init__(self, props, quality, max_window_bits=0, strategy=0):
        # the settings constructor  :108-109
        max_chain, lazy = get_max_chain(quality), 3 + quality // 3
        hash_bits, chain_size_bits = 15 + math.isqrt(2 * quality), 17 + math.isqrt(2 * quality)
        no_self_overlap, use_min_table = bool(strategy & 1), quality >= 10
        props = list(props)
        assert props and max_chain > 0 and 14 <= hash_bits <= 24
        self.props = props if len(props) != 1 else None                     # :52-53
        self.min_len = min(p.MinLength for p in props)                      # :56-68
        self.max_len = max(p.MaxLength for p in props)
        self.min_dist = min(p.MinDistance for p in props)
        self.max_dist = max(p.MaxDistance for p in props)
        windows_bits = max([1] + [p.WindowsBits for p in props])
        if max_window_bits != 0:                                            # :69-73
            windows_bits = max(windows_bits, max_window_bits)
            self.max_dist = max(self.max_dist, 1 << max_window_bits)
        self.lazy, self.no_self_overlap = lazy, no_self_overlap
        self.hash_bits, self.hash_mask = hash_bits, (1 << hash_bits) - 1
        self.head = [-1] * (1 << hash_bits)
        self.max_chain = max_chain
        if max_chain == 1:                                                  # :86-91
            self.chain, self.chain_mask = [-1], 0
        else:
            chain_size_bits = min(chain_size_bits, windows_bits)           # :94-96
            self.chain, self.chain_mask = [-1] * (1 << chain_size_bits), (1 << chain_size_bits) - 1
        self.min_mask, self.min_table = 0, None
        if use_min_table and self.min_len < 4:                              # :100-104
            self.min_mask = M32 >> ((4 - self.min_len) * 8)
            self.min_table = [-1] * 0x10000
        self.position = 0
        self._hashed = None

    def _hashes(self, data):
        """ComputeHash  :288-299 for every position that has four bytes"""
        if self._hashed is not data:
            n = len(data)
            if n >= 4:
                a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
                v = a[:n - 3] | (a[1:n - 2] << 8) | (a[2:n - 1] << 16) | (a[3:] << 24)
                self.h4 = ((((v * PRIME) & M32) >> (32 - self.hash_bits)) & self.hash_mask).tolist()
                self.hm = (((((v & self.min_mask) * PRIME) & M32) >> 16) & 0xFFFF).tolist()
            else:
                self.h4, self.hm = [], []
            self._hashed = data

    def _insert(self, pos, h4, hm):      # :134-144
        if self.chain_mask != 0:
            self.chain[pos & self.chain_mask] = self.head[h4]
        self.head[h4] = pos
        if self.min_table is not None:
            self.min_table[hm] = pos

    def _score(self, length, distance):
        """ScoreMatch  :301-321 -> (score, length)"""
        if self.no_self_overlap and length > distance:
            length = distance
        if self.props is None:
            return length - self.min_len, length
        for p in self.props:
            if distance <= p.MaxDistance and length >= p.MinLength and distance >= p.MinDistance:
                if length > p.MaxLength:
                    length = p.MaxLength
                return length - p.MinLength, length
        return -1, 0

    def _chain_matches(self, data, best_possible, pos, cur, attempts):
        """ChainMatches  :248-282 -> (distance, length): a candidate nearer than minDistance is skipped but has used its attempt"""
        best_d = best_l = 0
        best_score = -1
        chain, mask = self.chain, self.chain_mask
        while cur != -1 and attempts > 0:
            attempts -= 1
            distance = pos - cur
            if distance > self.max_dist:
                break
            if distance < self.min_dist:
                cur = chain[cur & mask]
                continue
            score, ln = self._score(match_length(data, pos, cur, best_possible), distance)
            if score > best_score:
                best_score, best_l, best_d = score, ln, distance
                if best_l == best_possible:
                    break
            cur = chain[cur & mask]
        return best_d, best_l

    def _match_search(self, data, pos, attempts):
        """MatchSearch  :214-246"""
        h4, hm = self.h4[pos], self.hm[pos]
        best_possible = min(len(data) - pos, self.max_len)
        best_d, best_l = self._chain_matches(data, best_possible, pos, self.head[h4], attempts)
        if best_l == 0 and self.min_table is not None:                      # the fallback for small matches  :226-243
            cur = self.min_table[hm]
            if cur != -1:
                distance = pos - cur
                if distance < self.min_dist:
                    distance = self.min_dist
                # (pos - distance >= 0 is the oracle's guard and the kernels': after the clamp the managed code would read in front of the span --
                # undefined; such a candidate counts as none)
                if distance <= self.max_dist and pos - distance >= 0:
                    _, best_l = self._score(match_length(data, pos, pos - distance, best_possible), distance)
                    best_d = distance
        self._insert(pos, h4, hm)
        return best_d, best_l

    def find_next_best_match(self, data):
        """FindNextBestMatch  :157-212"""
        self._hashes(data)
        length = len(data)
        limit = length - 4
        while self.position <= limit:
            best_d, best_l = self._match_search(data, self.position, self.max_chain)
            if best_l < self.min_len:
                self.position += 1
                continue
            skip = 0
            if best_l <= self.lazy and self.position + 1 <= limit:          # lazy matching  :176-190
                next_d, next_l = self._match_search(data, self.position + 1, self.max_chain)
                if next_l > best_l:
                    best_l, best_d = next_l, next_d
                    self.position += 1
                else:
                    skip += 1
            match = (self.position, best_d, best_l)
            end = self.position + best_l                                    # fill the hash window  :196-203
            self.position += 1 + skip
            h4, hm = self.h4, self.hm
            while self.position < end and self.position <= limit:
                self._insert(self.position, h4[self.position], hm[self.position])
                self.position += 1
            return match
        self.position = length
        return (length, 0, 0)


def matches(props, data, quality, max_window_bits=0, strategy=0):
    data = bytes(data)
    f = ChainFinder(props if isinstance(props, (list, tuple)) else [props], quality, max_window_bits, strategy)
    out = []
    while True:
        m = f.find_next_best_match(data)
        out.append(m)
        if m[2] == 0:
            return out


class FlagWriter:
    """FlagWriter(destination, bit order) with 8-bit flags  FlagWriter.cs:13-147: payload waits in Buffer until its flag byte is complete"""

    def __init__(self, msb_first):
        self.out, self.buffer = bytearray(), bytearray()
        self.msb, self.left, self.cur = msb_first, 8, 0

    def write_bit(self, bit):            # :70-80
        if bit:
            self.cur |= 1 << (self.left - 1 if self.msb else 8 - self.left)
        self.left -= 1
        if self.left == 0:
            self.flush()

    def write_int(self, value, bits):    # :90-98 (reverseOrder false: least significant bit first)
        for i in range(bits):
            self.write_bit((value >> i) & 1)

    def flush(self):                     # :111-127
        if self.left != 8:
            self.out.append(self.cur)
            self.left, self.cur = 8, 0
        if self.buffer:
            self.out += self.buffer
            del self.buffer[:]

    def flush_if_necessary(self):        # :132-139
        if self.left == 8 and self.buffer:
            self.out += self.buffer
            del self.buffer[:]
