package com.github.tashoyan.recommender.deduplicator

import com.github.tashoyan.recommender.locrec.{LocrecBackend, LocrecNative}
import org.apache.spark.sql.functions.col
import org.apache.spark.sql.types.{DoubleType, LongType, StringType}
import org.apache.spark.sql.{DataFrame, Row}

import scala.collection.mutable.ArrayBuffer

/**
  * Drop-in replacement of the reference class of the same name and package
  * (recommender/src/main/scala/com/github/tashoyan/recommender/deduplicator/PlaceDeduplicator.scala:8-56): same
  * constructor, same method, same result - the places' columns of every (place, confirmed place of its region with
  * another id) pair that is not the same place, one row per pair.  The reference joins the two frames per region and
  * runs a UDF per pair; here the five columns of both frames are collected once, the names lower-cased with the JVM's
  * own `toLowerCase` (as the UDF does) and handed over as UTF-16 code units, and one native call finds the pairs that
  * ARE the same place with a grid join and a thresholded Levenshtein on the device.  The result frame is rebuilt from
  * the per-place counts of pairs that are not.  `LOCREC_BACKEND=spark` delegates to the reference's implementation
  * (renamed SparkPlaceDeduplicator, as its two siblings are).
  */
class PlaceDeduplicator(
    maxPlaceDistanceMeters: Double,
    maxNameDifference: Int
) {

  private lazy val sparkDelegate = new SparkPlaceDeduplicator(maxPlaceDistanceMeters, maxNameDifference)

  private class Side(val ids: Array[Long], val regionIds: Array[Long], val latitudes: Array[Double], val longitudes: Array[Double],
      val nameOffsets: Array[Long], val nameUnits: Array[Int])

  /** The five columns of the rows, names as CSR of lower-cased UTF-16 code units. A null name in a region the other frame
    * has rows in throws NullPointerException, as `name.toLowerCase` does inside the reference's UDF. */
  private def sideOf(rows: Array[Row], otherRegions: Set[Long]): Side = {
    val n = rows.length
    val ids = new Array[Long](n)
    val regionIds = new Array[Long](n)
    val latitudes = new Array[Double](n)
    val longitudes = new Array[Double](n)
    val offsets = new Array[Long](n + 1)
    val units = new ArrayBuffer[Int]()
    var i = 0
    while (i < n) {
      val row = rows(i)
      regionIds(i) = row.getLong(0)
      ids(i) = row.getLong(1)
      val name = if (row.isNullAt(2)) null else row.getString(2)
      if (name == null && otherRegions.contains(regionIds(i)))
        throw new NullPointerException(s"the name of the place with id ${ids(i)} is null")
      if (name != null) {
        val lower = name.toLowerCase
        var c = 0
        while (c < lower.length) {
          units += lower.charAt(c).toInt
          c += 1
        }
      }
      latitudes(i) = row.getDouble(3)
      longitudes(i) = row.getDouble(4)
      offsets(i + 1) = units.length.toLong
      i += 1
    }
    new Side(ids, regionIds, latitudes, longitudes, offsets, units.toArray)
  }

  private def fiveColumns(df: DataFrame): Array[Row] =
    df.select(
      col("region_id").cast(LongType),
      col("id").cast(LongType),
      col("name").cast(StringType),
      col("latitude").cast(DoubleType),
      col("longitude").cast(DoubleType)
    ).collect()

  def dropDuplicates(places: DataFrame, confirmedPlaces: DataFrame): DataFrame = if (LocrecBackend.useSpark) sparkDelegate.dropDuplicates(places, confirmedPlaces) else {
    val placeRows = places.collect()
    val placeColumns = fiveColumns(places)
    val confirmedColumns = fiveColumns(confirmedPlaces)
    require(placeRows.length == placeColumns.length, "places changed between two collects")
    val p = sideOf(placeColumns, confirmedColumns.map(_.getLong(0)).toSet)
    val c = sideOf(confirmedColumns, placeColumns.map(_.getLong(0)).toSet)
    val notSameCounts = new Array[Long](p.ids.length)
    // the pairs themselves are not needed for the literal result: arrays of length 0 only count them
    LocrecNative.dedupFindDuplicates(
      p.ids, p.regionIds, p.latitudes, p.longitudes, p.nameOffsets, p.nameUnits,
      c.ids, c.regionIds, c.latitudes, c.longitudes, c.nameOffsets, c.nameUnits,
      maxPlaceDistanceMeters, maxNameDifference,
      new Array[Long](0), new Array[Long](0), new Array[Int](0), notSameCounts
    )
    val out = new ArrayBuffer[Row]()
    var i = 0
    while (i < placeRows.length) {
      var t = 0L
      while (t < notSameCounts(i)) {
        out += placeRows(i)
        t += 1
      }
      i += 1
    }
    val spark = places.sparkSession
    spark.createDataFrame(spark.sparkContext.parallelize(out.toSeq, 1), places.schema)
  }

}
