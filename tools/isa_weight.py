"""tools/isa_weight.py FILE.s [DIGIT_LOOPS] — executed instructions per site of a generated lane kernel, from its listing: every
backward branch closes a loop; loops nested inside the chunk loop run 3 times per level (the looped members' digits).
DIGIT_LOOPS: the kernel's number of looped members — where more large loops are found, the outermost extra ones (the chrX
pass loop, which the once-per-site form's per-pass code makes large enough to be seen) run once.
Then, per loop depth, the exposed waits on the load/LDS counter and the lane spills of SGPRs (see below)."""
import re,sys,collections
f=sys.argv[1]
lines=[l for l in open(f).read().split('\n')]
addr={}
for i,l in enumerate(lines):
    m=re.search(r'// ([0-9A-F]{12}):',l)
    if m: addr[int(m.group(1),16)]=i
base=min(addr)
loops=[]
for i,l in enumerate(lines):
    m=re.search(r's_cbranch_\w+ (\d+)\s+// ([0-9A-F]{12}):.*<\w+\+0x([0-9a-f]+)>',l)
    if m:
        tgt=base+int(m.group(3),16); here=int(m.group(2),16)
        if tgt<here and tgt in addr: loops.append((addr[tgt],i))
loops.sort(key=lambda ab:(ab[0],-ab[1]))
# the chunk loop = the largest; digit loops = loops inside it with > 300 instructions
big=max(loops,key=lambda ab:ab[1]-ab[0])
digit=[ab for ab in loops if ab!=big and ab[0]>=big[0] and ab[1]<=big[1] and ab[1]-ab[0]>300]
extra=max(0,len(digit)-int(sys.argv[2])) if len(sys.argv)>2 else 0
once=sorted(digit,key=lambda ab:ab[0]-ab[1])[:extra]  # the largest: once per site
print("chunk loop",big,"digit loops",[ab for ab in digit if ab not in once],"once per site",once)
w=collections.Counter(); tot=0
kinds=collections.defaultdict(collections.Counter)
for i in range(big[0],big[1]+1):
    l=lines[i].strip()
    if not l or l.startswith('//') or ':' in l.split()[0]: continue
    d=sum(1 for a,b in digit if a<=i<=b and (a,b) not in once)
    w[d]+=1
    op=l.split()[0]
    k='fp64' if op.startswith(('v_fma','v_mul_f64','v_add_f64','v_div','v_rcp_f64')) else ('acc' if 'accvgpr' in op else ('lds' if op.startswith('ds_') else ('smem' if op.startswith('s_load') else ('wait' if op=='s_waitcnt' else 'other'))))
    kinds[d][k]+=1
N=len(digit)-len(once)
total=sum(c*3**d for d,c in w.items())
for d in sorted(w):
    print("depth",d,"static",w[d],"x",3**d,"=",w[d]*3**d,dict(kinds[d]))
print("executed per site ~",total,"; per configuration at 3^%d x block"%N)
# Exposed waits: every s_waitcnt on the load/LDS counter (lgkmcnt) with the number of instructions between it and the youngest
# load it covers (scalar loads and LDS reads; LDS writes count in the counter but are not waited for as data).  "entry": the loads
# outstanding when the listing is read top to bottom; "around": those outstanding when the wait is reached again through the
# back edge of the innermost loop that holds it (a load issued a whole step earlier).  A wave that runs alone on its SIMD parks
# for what is left of the load's latency, so a short distance is an exposed wait; the compiler decides the schedule, so this
# is a report and no test.  Lane spills of SGPRs (v_readlane / v_writelane) are counted per depth as well.
NEAR=8  # instructions: fewer than this between load and wait count as exposed (a scalar-cache hit or an LDS read takes tens of cycles)
def op_of(i):
    l=lines[i].strip()
    return '' if (not l or l.startswith('//') or ':' in l.split()[0]) else l.split()[0]
def lgkm_n(i):
    m=re.search(r'lgkmcnt\((\d+)\)',lines[i])
    return int(m.group(1)) if m and op_of(i)=='s_waitcnt' else None
def is_load(op): return op.startswith(('s_load','s_buffer_load','ds_read','ds_load'))
def counted(op): return is_load(op) or op.startswith('ds_')
def walk(path,target):
    """instructions of `path` in order -> (distance, load op) of the youngest load covered by the wait at the LAST element"""
    out=[]  # outstanding: (position in path, op)
    for pos,i in enumerate(path):
        op=op_of(i)
        if not op: continue
        n=lgkm_n(i)
        if n is not None:
            covered=out[:len(out)-n] if n else out
            if pos==len(path)-1:
                ld=[c for c in covered if is_load(c[1])]
                return (sum(1 for j in path[ld[-1][0]+1:pos] if op_of(j)),ld[-1][1]) if ld else (None,'-')
            out=out[len(out)-n:] if n else []
        elif counted(op): out.append((pos,op))
    return (None,'-')
print("exposed waits (lgkmcnt): distance in instructions to the youngest covered load, entry / around the innermost loop; near = < %d"%NEAR)
near=collections.Counter(); spills=collections.Counter(); allw=collections.Counter()
for i in range(big[0],big[1]+1):
    op=op_of(i)
    d=sum(1 for a,b in digit if a<=i<=b and (a,b) not in once)
    if op.startswith(('v_readlane','v_writelane')): spills[d]+=1
    if lgkm_n(i) is None: continue
    inner=[ab for ab in loops if ab[0]<=i<=ab[1]]
    a,b=min(inner,key=lambda ab:ab[1]-ab[0])
    e_dist,e_op=walk(list(range(a,i+1)),i)
    r_dist,r_op=walk(list(range(a,b+1))+list(range(a,i+1)),i)
    allw[d]+=1
    # the wait is exposed where the nearer of the two paths is: entry counts once per run of the loop, around on the other turns
    worst=min(x for x in (e_dist,r_dist,10**9) if x is not None)
    if worst<NEAR: near[d]+=1
    if d>0 or worst<NEAR:
        print("  depth %d line %d lgkmcnt(%d): entry %s %s, around %s %s%s"%(d,i+1,lgkm_n(i),e_dist,e_op,r_dist,r_op,"  <- near" if worst<NEAR else ""))
for d in sorted(set(allw)|set(spills)):
    print("depth",d,"waits",allw[d],"near",near[d],"x",3**d,"=",near[d]*3**d,"; v_readlane/v_writelane",spills[d])
print("near waits per site ~",sum(c*3**d for d,c in near.items()),"; lane spill instructions inside digit loops",sum(c for d,c in spills.items() if d>0))
