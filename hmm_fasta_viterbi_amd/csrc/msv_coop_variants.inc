// The cooperative variants, in table order: MSV_COOP_VARIANT(W, S), MSV_COOP_SPLIT_VARIANT(W, S, SA); the halo is
// 16 states rounded up to whole lanes, (16 + S - 1) / S * S.
// 448 / 960 / 1464 states with the whole table in LDS; 1984 / 2480 with the split table.
MSV_COOP_VARIANT(4, 2),
MSV_COOP_VARIANT(4, 4),
MSV_COOP_VARIANT(4, 6),
MSV_COOP_SPLIT_VARIANT(4, 8, 6),
MSV_COOP_SPLIT_VARIANT(4, 10, 6),
