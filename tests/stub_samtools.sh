#!/bin/sh
# Stands in for samtools (test infrastructure): the reference seqToProfile reads its input through
# `<samtools> view -F 0xD04 -q 20 <bam>`; this prints the file named by the last argument as it is, unfiltered,
# so the reference trains on the same SAM text the product's --sam route reads.
for last; do :; done
cat "$last"
