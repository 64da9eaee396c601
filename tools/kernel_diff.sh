#!/bin/bash
# Which kernels differ between two builds of the libnet2_sha2 kernels object:
# per kernel, the instruction text of the gfx950 disassembly (no addresses, no
# encodings) compared as plain text, with both instruction counts, and any
# differing resource line (VGPRs, SGPRs, spills, scratch, LDS size) of the
# code-object notes (kernel_res.sh prints those of one build).  A kernel whose
# text differs only in 32-bit literals is said so: a kernel that takes the
# address of a table pc-relative carries the distance as a literal, and that
# moves when a kernel placed before it changes length.
#   bash tools/kernel_diff.sh OLD.o NEW.o [-v]      -v: also the diff itself
# Exit status 0 whether or not anything differs; 2 on a usage error.
set -eu
[ $# -ge 2 ] || { echo "usage: $0 OLD.o NEW.o [-v]" >&2; exit 2; }
B=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT

unpack() {	# object, tag: $T/tag.asm (one directory of per-kernel texts), $T/tag.res
	$B/llvm-objcopy --dump-section=.hip_fatbin="$T/$2.fat" "$1" "$T/$2.tmp.o"
	$B/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
	    --input="$T/$2.fat" --output="$T/$2.co" --unbundle
	mkdir "$T/$2.asm"
	$B/llvm-objdump -d --no-show-raw-insn --no-leading-addr "$T/$2.co" |
	  sed -e 's#[[:space:]]*//.*$##' |
	  awk -v dir="$T/$2.asm" '
	    /^<.*>:$/ { name = substr($0, 2, length($0) - 3); next }
	    name != "" && /^\t/ { print > (dir "/" name) }'
	$B/llvm-readelf --notes "$T/$2.co" |
	  grep -E "^ +\.name:|\.vgpr_count:|\.sgpr_count:|\.vgpr_spill_count|\.sgpr_spill_count|\.private_segment_fixed_size|\.group_segment_fixed_size" |
	  awk '$1 == ".name:" { name = $2 }
	       $1 != ".name:" { v[$1] = $2 }
	       $1 == ".vgpr_spill_count:" {	# the last of a kernel'"'"'s lines
	         print name, "vgpr", v[".vgpr_count:"], "sgpr", v[".sgpr_count:"],
	           "lds", v[".group_segment_fixed_size:"],
	           "scratch", v[".private_segment_fixed_size:"],
	           "spills", v[".vgpr_spill_count:"] "+" v[".sgpr_spill_count:"] }' |
	  sort > "$T/$2.res"
}
unpack "$1" old
unpack "$2" new

report() {
same=0 differ=0 lits=0
LIT='s/0x[0-9a-f]{8}$/LITERAL/'
for f in $( (ls "$T/old.asm"; ls "$T/new.asm") | sort -u); do
	if [ ! -f "$T/old.asm/$f" ] || [ ! -f "$T/new.asm/$f" ]; then
		echo "only in $([ -f "$T/old.asm/$f" ] && echo old || echo new): $f"
		differ=$((differ + 1))
	elif cmp -s "$T/old.asm/$f" "$T/new.asm/$f"; then
		same=$((same + 1))
	else
		if cmp -s <(sed -E "$LIT" "$T/old.asm/$f") <(sed -E "$LIT" "$T/new.asm/$f"); then
			lits=$((lits + 1))
			echo "32-bit literals only: $f  lines $(diff "$T/old.asm/$f" "$T/new.asm/$f" | grep -c '^>')"
		else
			differ=$((differ + 1))
			echo "differs: $f  instructions $(wc -l < "$T/old.asm/$f") -> $(wc -l < "$T/new.asm/$f")"
		fi
		if [ "$1" = -v ]; then
			diff "$T/old.asm/$f" "$T/new.asm/$f" || true
		fi
	fi
done
echo "kernels: $same identical in disassembly, $lits but for 32-bit literals, $differ not"
echo "resource lines, old above new:"
diff "$T/old.res" "$T/new.res" | grep '^[<>]' || echo "  all $(wc -l < "$T/new.res") identical"
}
# readable names: demangled, without the parameter lists
report "${3:-}" | c++filt | sed -E 's/\((unsigned|void|Net2|net2)[^()]*\)//; s/net2::dev:://g'
