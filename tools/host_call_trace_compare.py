"""Compare two rocprofv3 output directories (hip api + kernel + memory-copy traces, csv): ordered HIP API names of the main
thread, and -- joined through the correlation id -- the stream of every launch and copy, normalised by first appearance."""
import csv
import glob
import sys
from collections import Counter


def one(d, pat):
    f = glob.glob(d + "/**/*" + pat, recursive=True)
    return f[0] if f else None


def load(d):
    api = list(csv.DictReader(open(one(d, "hip_api_trace.csv"))))
    print(d, "hip api columns:", list(api[0].keys()))
    api = [r for r in api if not r["Function"].startswith("__hip")]
    tid = Counter(r["Thread_Id"] for r in api).most_common(1)[0][0]
    other = [r for r in api if r["Thread_Id"] != tid]
    api = sorted((r for r in api if r["Thread_Id"] == tid), key=lambda r: int(r["Start_Timestamp"]))
    stream = {}
    for pat in ("kernel_trace.csv", "memory_copy_trace.csv"):
        f = one(d, pat)
        if not f:
            print(d, "no", pat)
            continue
        rows = list(csv.DictReader(open(f)))
        if rows:
            print(d, pat, "columns:", list(rows[0].keys()))
        for r in rows:
            if "Stream_Id" in r:
                stream[r["Correlation_Id"]] = r["Stream_Id"]
    norm, seq = {}, []
    for r in api:
        s = stream.get(r["Correlation_Id"])
        if s is not None:
            s = norm.setdefault(s, len(norm))
        seq.append((r["Function"], s))
    return seq, len(other), len(norm)


a, oa, na = load(sys.argv[1])
b, ob, nb = load(sys.argv[2])
print("calls: %d against %d; on other threads %d / %d; distinct streams seen %d / %d" % (len(a), len(b), oa, ob, na, nb))
print("calls with a stream: %d / %d" % (sum(s is not None for _, s in a), sum(s is not None for _, s in b)))
print("top names:", Counter(n for n, _ in a).most_common(12))
same = len(a) == len(b)
for i, (x, y) in enumerate(zip(a, b)):
    if x != y:
        same = False
        print("FIRST DIFFERENCE at call", i, x, y)
        print(" before:", a[max(0, i - 8):i])
        print(" parent next:", a[i:i + 8])
        print(" change next:", b[i:i + 8])
        break
print("IDENTICAL" if same else "DIFFERENT")
sys.exit(0 if same else 1)
