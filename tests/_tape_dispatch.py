"""The dispatch record of csrc/tape.hip: oracle/_build/tape_dispatch (tape.hip compiled for the host, linked with recording stand-ins
for every entry point) replays raw wire vectors and prints the call run_one() makes for each - tests/test_tape_dispatch_cpu.py
compares that with tests/golden/tape_dispatch.json.

    python -m tests._tape_dispatch --record      appends the cases of the working tree's table that are not on record yet (a new op, a
                                                 new optional form) with what the working tree's tape.hip makes of them, and rewrites
                                                 the codes and the schema dump; records already in the file are never re-recorded -
                                                 one that no longer holds fails the test and is changed by hand, deliberately
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "oracle", "_build", "tape_dispatch")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tape_dispatch.json")
N_I, N_F, N_P = 15, 4, 12
STREAM = 0x99                       # what the driver passes as the stream


def replay(vectors, program=None):
    """One record (the recorder's output lines, joined by '; ') per raw vector [code, i[15], f[4], n, p[12]]."""
    if program is None:
        program = PROGRAM
        if not os.path.exists(program):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "_build/tape_dispatch", "PYTHON=" + sys.executable],
                           check=True, capture_output=True)
    text = "\n".join(" ".join([str(code), *map(str, i), *(float(v).hex() for v in f), str(n), *map(str, p)]) for code, i, f, n, p in vectors)
    out = subprocess.run([program], input=text + "\n", capture_output=True, text=True, check=True).stdout
    records, cur = [], []
    for line in out.splitlines():
        cur.append(line)
        if line.startswith("rc "):
            records.append("; ".join(cur))
            cur = []
    assert not cur and len(records) == len(vectors), (len(records), len(vectors), cur)
    return records


def schema_dump(schema):
    return {code: dict(i=list(s.i), p=list(s.p), f=list(s.f), writes=list(s.writes), opts=list(s.opts), b16=list(s.b16)) for code, s in schema.items()}


def cases(schema, codes):
    """The raw vectors of the record, chosen from the table: per op a base case (ordinary i slots 100 + k, f 0.5 + k, n 777, its p slots
    0x1000 + 16 k), each i slot zeroed and each p slot nulled in turn, each opts slot at 1, 2, 3, every non-zero b16 word (the
    convolutions at ks 1 and 3), the slab-count check of the weight gradient, and the two codes next to the valid range."""
    out, seen = [], set()

    def add(code, i, f, n, p):
        key = (code, tuple(i), tuple(f), n, tuple(p))
        if key not in seen:
            seen.add(key)
            out.append([code, list(i), list(f), n, list(p)])

    f = [0.5 + k for k in range(N_F)]
    for name, s in schema.items():
        code = codes[name]
        special = set(s.opts) | {"b16"} | {nm for nm in s.i if nm.startswith("rsv")}
        base_i = [100 + k if k < len(s.i) and s.i[k] not in special else 0 for k in range(N_I)]
        base_p = [0x1000 + 16 * k if k < len(s.p) else 0 for k in range(N_P)]

        def put(i=None, p=None):
            vi, vp = list(base_i), list(base_p)
            for nm, v in (i or {}).items():
                vi[s.ix[nm]] = v
            for nm in p or ():
                vp[s.px[nm]] = 0
            add(code, vi, f, 777, vp)

        put()
        for nm in s.i:
            if nm not in special:
                put(i={nm: 0})
        for nm in s.p:
            put(p=[nm])
        for nm in s.opts:
            for v in (1, 2, 3):
                put(i={nm: v})
        for word in range(1, 1 << len(s.b16)):
            if "ks" in s.ix:
                put(i={"b16": word, "ks": 1})
                put(i={"b16": word, "ks": 3})
            else:
                put(i={"b16": word})
        if name == "UZ_OP_CONV_BWD_WEIGHT":
            put(i={"slabs_only": 1, "nslab": 0})
            put(i={"slabs_only": 1, "nslab": 5})          # the stand-in answers 0 slabs: the refusal, its message part of the record
    for code in (0, codes["UZ_OP__COUNT"]):
        add(code, [0] * N_I, f, 777, [0] * N_P)
    return out


def record():
    import unet_zoo_amd  # noqa: F401
    from unet_zoo_amd import _ffi, _ops
    codes = _ffi.op_codes()
    old = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else dict(records=[], schema={})
    kept = old["records"]                                                            # what is on record stays as recorded
    have = {json.dumps(v) for v, _ in kept}
    new = [v for v in cases(_ops.SCHEMA, codes) if json.dumps(v) not in have]
    vectors, records = [v for v, _ in kept] + new, [r for _, r in kept] + replay(new)
    dump = schema_dump(_ops.SCHEMA)
    order = [code for code in old["schema"] if code in dump] + [code for code in dump if code not in old["schema"]]
    one = lambda v: json.dumps(v, separators=(",", ":"))
    with open(GOLDEN, "w") as fh:
        fh.write('{"codes": ' + json.dumps(codes) + ',\n"schema": {\n')
        fh.write(",\n".join(f"{json.dumps(code)}: {json.dumps(s)}" for code, s in ((code, dump[code]) for code in order)))
        fh.write('},\n"records": [\n')
        fh.write(",\n".join(f"[{one(v)},{json.dumps(r)}]" for v, r in zip(vectors, records)))
        fh.write("]}\n")
    print(f"{len(records)} records -> {GOLDEN}")


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    else:
        sys.exit(__doc__)
