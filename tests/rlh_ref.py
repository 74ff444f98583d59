"""Pure-Python restatement of the three RLE / Huffman decoders of the Nintendo GBA / DS family and of the RLE30 encoder, as the independent
check of the alz_rlh_* entry points (the C oracle has no such body).  Paths are relative to the reference's src/AuroraLib.Compression.Nintendo.
Pinned by hand-assembled known answers (tests/golden/make_kats_rlh.py).  Also a TEST-ONLY HUF20 stream builder (the managed encoder's output is
not a function of its input: DESIGN.md 7).

Every decoder returns (bytes written at dst_off, status, dst_len, src_used); src_used is None where the header leaves it unspecified
(OUTPUT_CAPACITY)."""
OK, INPUT_TRUNCATED, OUTPUT_SIZE_MISMATCH, OUTPUT_CAPACITY, BAD_TOKEN = 0, 1, 2, 3, 4
RLH_RLE30, RLH_HUF20_4, RLH_HUF20_8 = 0, 1, 2


def rle30_decode(src, decom_len, cap):
    """RLE30.DecompressHeaderless  Nintendo/RLE30.cs:76-105; E5 as the LZ10 body."""
    src = bytes(src)
    out = bytearray()
    p = 0
    while len(out) < decom_len:                                   # :82
        if p >= len(src):                                         # ReadByte() = -1 -> a literal run of 128 that cannot be read  :84-96
            return bytes(out), INPUT_TRUNCATED, len(out), len(src)
        c = src[p]
        n = (c & 0x7F) + 1                                        # :85
        if c >= 0x80:                                             # :87-91
            if p + 1 >= len(src):
                return bytes(out), INPUT_TRUNCATED, len(out), len(src)
            tok = bytes([src[p + 1]]) * (n + 2)
            p += 2
        else:                                                     # :92-97 (read into a temporary: a short run is never written)
            if p + 1 + n > len(src):
                return bytes(out), INPUT_TRUNCATED, len(out), len(src)
            tok = src[p + 1:p + 1 + n]
            p += 1 + n
        if len(out) + len(tok) > cap:                             # E5: the token that would exceed dst_cap is clipped and ends decoding
            end = len(out) + len(tok)
            out += tok[:cap - len(out)]
            if end > decom_len and cap >= decom_len:
                return bytes(out), OUTPUT_SIZE_MISMATCH, len(out), p
            return bytes(out), OUTPUT_CAPACITY, len(out), None
        out += tok                                                # :98
    if len(out) > decom_len:                                      # :101-104
        return bytes(out), OUTPUT_SIZE_MISMATCH, len(out), p
    return bytes(out), OK, len(out), p


def _rel_match_length(data):
    """RleMatchFinder.GetRelMatchLength  MatchFinder/RleMatchFinder.cs:53-64"""
    for i in range(1, len(data)):
        if data[i] != data[0]:
            return i
    return len(data)


def rle30_encode(src, min_match=3, max_match=127):
    """RLE30.CompressHeaderless  Nintendo/RLE30.cs:110-129 over RleMatchFinder.TryToFindMatch (RleMatchFinder.cs:29-51), defect included:
    `duration = source.Length - offset` (:43) lets a literal run reach max_match + 2 = 129 bytes, whose control byte wraps to 0x80."""
    src = bytes(src)
    out = bytearray()
    p = 0
    while p < len(src):
        duration = _rel_match_length(src[p:p + min(max_match, len(src) - p)])     # :31-32
        if duration < min_match:                                                  # :34
            duration = 0
            while True:
                duration += 1                                                     # :39
                if len(src) - p - duration < min_match:                           # :41-45
                    duration = len(src) - p
                    break
                if duration == max_match or _rel_match_length(src[p + duration:p + duration + min_match]) == min_match:   # :46-47
                    break
            out.append((duration - 1) & 0xFF)                                     # RLE30.cs:124
            out += src[p:p + duration]
        else:
            out.append(((duration - 3) | 0x80) & 0xFF)                            # RLE30.cs:119-120
            out.append(src[p])
        p += duration
    return bytes(out)


def rle30_encode_bound(n):
    """every token spends one control byte on at least one input byte"""
    return 2 * n


def huf20_decode(src, decom_len, cap, bit_depth, big=False):
    """HUF20.DecompressHeaderless  Nintendo/HUF20.cs:94-152.  dst_len = 0 for every non-OK status (:103-107: the destination receives the
    buffer only after the whole decode succeeded)."""
    src = bytes(src)
    if len(src) < 2:                                              # ReadUInt8 x 2  :98-99
        return b"", INPUT_TRUNCATED, 0, len(src)
    tree_size, root = src[0], src[1]
    tree = bytearray(tree_size * 2)                               # :100
    got = src[2:2 + tree_size * 2]                                # :101 -- a short Read leaves zeros and is no error
    tree[:len(got)] = got
    p = 2 + len(got)
    out = bytearray(decom_len)                                    # :122 (cleared; the 8-bit path overwrites)
    symbols = decom_len * 8 // bit_depth                          # :117
    flag = bits_left = nxt = i = 0
    pos = root
    little = not big
    while i < symbols:                                            # :124
        if bits_left == 0:                                        # :126-130
            if p + 4 > len(src):
                return b"", INPUT_TRUNCATED, 0, len(src)
            flag = int.from_bytes(src[p:p + 4], "little")
            p += 4
            bits_left = 32
        nxt += ((pos & 0x3F) << 1) + 2                            # :132
        bits_left -= 1
        direction = 2 - ((flag >> bits_left) & 1)                 # :133
        leaf = (pos >> (5 + direction)) & 1                       # :134
        if nxt - direction >= len(tree):                          # :136 IndexOutOfRangeException
            return b"", INPUT_TRUNCATED, 0, p
        pos = tree[nxt - direction]
        if leaf:
            if bit_depth == 8:
                out[i] = pos                                      # :141
            else:
                shift = ((i & 1) == 0) ^ little                   # :145
                out[i // 2] |= (pos << (4 if shift else 0)) & 0xFF    # :146 -- the WHOLE tree byte
            i += 1
            pos = root                                            # :148-149
            nxt = 0
    if cap < decom_len:
        return b"", OUTPUT_CAPACITY, 0, None
    return bytes(out), OK, decom_len, p


class _Node:
    def __init__(self, freq, sym=None, left=None, right=None):
        self.freq, self.sym, self.left, self.right, self.value = freq, sym, left, right, 0

    @property
    def leaf(self):
        return self.left is None


def huf20_label(root):
    """HUF20.BuildLabelTreeList (HUF20.cs:202-246) + the header it is written as (:159-165): treeSize, treeRoot, one byte pair per labelled
    node.  None when a 6-bit offset would overflow (or the list outgrows the size byte)."""
    labels, pending = [], [root]
    while pending:                                                # :213-244
        k = min(range(len(pending)), key=lambda j: (pending[j].value - j, j))   # lowest Score = Value - i, first on ties (OrderBy is stable)
        node = pending.pop(k)
        node.value = len(labels) - node.value                     # :222
        if node.value > 0x3F:
            return None
        labels.append(node)
        if node.left.leaf:
            node.value |= 0x80
        else:
            node.left.value = len(labels)
            pending.append(node.left)
        if node.right.leaf:
            node.value |= 0x40
        else:
            node.right.value = len(labels)
            pending.append(node.right)
    if len(labels) > 255:
        return None
    out = bytearray([len(labels), labels[0].value])               # :159-160
    for n in labels:                                              # :161-165
        out.append(n.left.sym if n.left.leaf else n.left.value)
        out.append(n.right.sym if n.right.leaf else n.right.value)
    return out


def huf20_tree(freq, bit_depth):
    """Huffman tree of {symbol: frequency} by a STABLE sort on frequency, laid out as HUF20.BuildLabelTreeList does (HUF20.cs:202-246).
    Returns (treeSize + treeRoot + tree bytes, {symbol: (code, length)}); None when a 6-bit offset would overflow."""
    nodes = [_Node(f, s) for s, f in sorted(freq.items())]
    if not nodes:
        nodes = [_Node(0, 0)]
    if len(nodes) == 1:
        nodes.append(_Node(0, (nodes[0].sym + 1) & ((1 << bit_depth) - 1)))     # (a second leaf: the decoder needs a node above a leaf)
    while len(nodes) > 1:
        nodes.sort(key=lambda n: n.freq)                          # list.sort is stable
        a, b = nodes[0], nodes[1]
        nodes = nodes[2:] + [_Node(a.freq + b.freq, None, a, b)]
    root = nodes[0]
    out = huf20_label(root)
    if out is None:
        return None
    codes = {}
    stack = [(root, 0, 0)]
    while stack:
        n, code, ln = stack.pop()
        if n.leaf:
            codes[n.sym] = (code, ln)
        else:
            stack.append((n.left, code << 1, ln + 1))             # bit 0 = left  (direction 2, :133-136)
            stack.append((n.right, (code << 1) | 1, ln + 1))
    return bytes(out), codes


def huf20_build(data, bit_depth, big=False):
    """TEST-ONLY builder of a valid HUF20 stream for `data` (huf20_tree + the code words), nibble order as the decoder reads it.
    None when a 6-bit offset would overflow."""
    data = bytes(data)
    little = not big
    if bit_depth == 8:
        syms = list(data)
    else:
        syms = []
        for b in data:
            lo, hi = b & 0xF, b >> 4
            syms += [lo, hi] if little else [hi, lo]              # decoder: symbol 2k goes to the low nibble in little order  :145
    freq = {}
    for s in syms:
        freq[s] = freq.get(s, 0) + 1
    tree = huf20_tree(freq, bit_depth)
    if tree is None:
        return None
    out, codes = bytearray(tree[0]), tree[1]
    acc = nbits = 0
    for s in syms:                                                # 32-bit words, MSB first, stored little-endian  (:128, :133)
        code, ln = codes[s]
        acc = (acc << ln) | code
        nbits += ln
        while nbits >= 32:
            out += ((acc >> (nbits - 32)) & 0xFFFFFFFF).to_bytes(4, "little")
            nbits -= 32
            acc &= (1 << nbits) - 1
    if nbits:
        out += ((acc << (32 - nbits)) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(out)


def decode(fmt, src, decom_len, cap, aux0=0):
    if fmt == RLH_RLE30:
        return rle30_decode(src, decom_len, cap)
    return huf20_decode(src, decom_len, cap, 4 if fmt == RLH_HUF20_4 else 8, big=bool(aux0) and fmt == RLH_HUF20_4)


def gba_header(type_byte, size):
    """type + u24 LE size, or type + u24 0 + u32 LE size  (RLE30.cs:62-71, HUF20.cs:80-88)"""
    if size <= 0xFFFFFF:
        return bytes([type_byte]) + size.to_bytes(3, "little")
    return bytes([type_byte, 0, 0, 0]) + size.to_bytes(4, "little")
